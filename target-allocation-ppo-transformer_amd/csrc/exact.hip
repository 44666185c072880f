// exact.hip -- the optimum of J(X) by a subset DP over the UAVs (uavhip_solve_exact), N <= 16. The
// rule, the feasible set and the tie-break are in include/uavhip.h. Built with -ffp-contract=off like
// the searches: J, covered and the ids of the result come from RefineRow::finish, k_refine's own code.
//
//   D_0[S] = 0;  D_{t+1}[S] = max over feasible T <= S of D_t[S \ T] + val_t(T);  J* = D_M[full]
//
// Three kernels per chunk of rows, all stream-ordered on one workspace:
//   k_exact_prepare    one wave per row: the id conversion (RefineRow::convert), then per target the
//                      masks of the UAVs that may be on it / must be on it and its capacity, and stats;
//   k_exact_stage      one launch per target t: D_t -> D_{t+1} and choice_t, one wave per tile;
//   k_exact_backtrack  one wave per row: t = M-1..0, T = choice_t[S], S <- S \ T, then finish.
//
// A stage's tile: the UAV bits split into L = min(N, 10) low and H = N - L high bits, and one wave
// (one 64-thread workgroup) owns the 2^L states of one high part Sh. It loops over the feasible
// Th <= Sh (descending), and per Th keeps in LDS
//   tile[Sl]  = D_t[Sh \ Th][Sl]                                   (staged, 8 KB)
//   comb[Tl]  = val_t(Th | Tl) = (v - w ch[Th]) - (v qh[Th]) ql[Tl] - w cl[Tl], -inf over capacity (8 KB)
// so one step of the maximisation is two LDS reads and an add: cand = tile[Sl ^ Tl] + comb[Tl]. The
// running maximum and its T of every state live in LDS across the Th (accv 8 KB, accc 2 KB).
//
// Lane balance. A state with k free bits has 2^k submasks: 3^L steps over 2^L states, the fullest 2^L.
// One state per lane in index order would leave a wave waiting on its fullest lane ((3/4)^6 = 18 % of
// the lanes busy over 64 consecutive states). Here every lane walks a LIST of states in one flattened
// loop (a step is one submask; at the last submask of a state the lane commits and takes its next
// state), and the lists are built at compile time by longest-processing-time-first over the states in
// descending popcount, so the lanes' step totals are equal to within the largest state: at L = 10 the
// fullest lane runs 1024 steps against a mean of 3^10 / 64 = 923 (90 % lane use); DESIGN.md 9i.
#include "refine_device.hpp"

namespace uavhip {
namespace {

constexpr int kExactLowBits = 10;
constexpr int kExactTile = 1 << kExactLowBits;

struct ExactMask {
    uint16_t may, must;  // bit u: UAV u may be on the target (free and allowed, or fixed to it) / is fixed to it
    int32_t cap;         // max(capacity, fixed UAVs on it); N without a capacity array
};

struct ExactLayout {
    long long d_bytes, choice_off, mask_off, row_bytes;
};
inline ExactLayout exact_layout(int N, int M) {
    ExactLayout w;
    w.d_bytes = (long long)sizeof(double) << N;
    w.choice_off = 2 * w.d_bytes;
    w.mask_off = (w.choice_off + ((long long)M * (long long)sizeof(uint16_t) << N) + 7) & ~7ll;
    w.row_bytes = (w.mask_off + (long long)M * (long long)sizeof(ExactMask) + 15) & ~15ll;
    return w;
}

// ------------------------------------------------------------------ the lanes' state lists
// States of L bits in descending popcount, each given to the lane with the fewest steps so far (the
// lowest such lane); lane l walks list[off[l]] .. list[off[l + 1] - 1].
template <int L>
struct ExactSched {
    uint16_t off[kWave + 1];
    uint16_t list[1 << L];
};
template <int L>
constexpr ExactSched<L> make_exact_sched() {
    ExactSched<L> s{};
    int load[kWave] = {}, count[kWave] = {};
    uint16_t lane_of[1 << L] = {};
    for (int k = L; k >= 0; --k)
        for (int st = 0; st < (1 << L); ++st) {
            int pc = 0;
            for (int b = 0; b < L; ++b) pc += st >> b & 1;
            if (pc != k) continue;
            int best = 0;
            for (int l = 1; l < kWave; ++l)
                if (load[l] < load[best]) best = l;
            load[best] += 1 << k;
            ++count[best];
            lane_of[st] = (uint16_t)best;
        }
    int at = 0;
    for (int l = 0; l < kWave; ++l) {
        s.off[l] = (uint16_t)at;
        at += count[l];
    }
    s.off[kWave] = (uint16_t)at;
    int fill[kWave] = {};
    for (int k = L; k >= 0; --k)  // a lane's own list in descending popcount too
        for (int st = 0; st < (1 << L); ++st) {
            int pc = 0;
            for (int b = 0; b < L; ++b) pc += st >> b & 1;
            if (pc != k) continue;
            const int l = lane_of[st];
            s.list[s.off[l] + fill[l]++] = (uint16_t)st;
        }
    return s;
}
#define UAVHIP_EXACT_SCHED(L) __device__ const ExactSched<L> g_exact_sched_##L = make_exact_sched<L>();
UAVHIP_EXACT_SCHED(1) UAVHIP_EXACT_SCHED(2) UAVHIP_EXACT_SCHED(3) UAVHIP_EXACT_SCHED(4) UAVHIP_EXACT_SCHED(5)
UAVHIP_EXACT_SCHED(6) UAVHIP_EXACT_SCHED(7) UAVHIP_EXACT_SCHED(8) UAVHIP_EXACT_SCHED(9) UAVHIP_EXACT_SCHED(10)

__device__ __forceinline__ void exact_sched(int L, const uint16_t*& off, const uint16_t*& list) {
#define UAVHIP_EXACT_PICK(K)         \
    case K:                          \
        off = g_exact_sched_##K.off; \
        list = g_exact_sched_##K.list; \
        break;
    switch (L) {
        UAVHIP_EXACT_PICK(1) UAVHIP_EXACT_PICK(2) UAVHIP_EXACT_PICK(3) UAVHIP_EXACT_PICK(4) UAVHIP_EXACT_PICK(5)
        UAVHIP_EXACT_PICK(6) UAVHIP_EXACT_PICK(7) UAVHIP_EXACT_PICK(8) UAVHIP_EXACT_PICK(9)
        default:
            off = g_exact_sched_10.off;
            list = g_exact_sched_10.list;
    }
}

// ------------------------------------------------------------------ prepare
// Row s0 + r: ids -> list indices, the per-target masks into the row's workspace, and stats =
// (invalid input ids, fixed_conflicts as pass 1 of the constrained search counts them).
template <int TPL, int NCAP>
__global__ __launch_bounds__(64 * kRefineWaves) void k_exact_prepare(
    uavhip_env env, int stride, int s0, int R, const uint8_t* __restrict__ allowed, const uint8_t* __restrict__ fixed,
    const int* __restrict__ capacity, const int* ain, char* __restrict__ ws, long long row_bytes, long long mask_off,
    int* __restrict__ stats) {
    const int r = blockIdx.x * kRefineWaves + (threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    if (r >= R) return;
    const int s = s0 + r;
    RefineRow<TPL, NCAP> row;
    row.load(env, s, stride, lane);
    row.convert(ain, s);
    const int N = row.N, M = row.M;
    const unsigned long long fx = ballot(fixed && row.isu && fixed[(long long)s * N + lane]);
    const uint8_t* al = allowed ? allowed + (long long)s * N * M : nullptr;
    const int* cp = capacity ? capacity + (long long)s * M : nullptr;

    int conflicts = 0;
    unsigned may[TPL], must[TPL];
#pragma unroll
    for (int j = 0; j < TPL; ++j) may[j] = must[j] = 0;
    for (int u = 0; u < N; ++u) {
        const int au = readlane_i(row.a, u);
        const bool isfx = fx >> u & 1;
        if (isfx && au >= 0) {
            // the fixed UAVs below u on the same target: n[a[u]] of pass 1
            const int before = __popcll(ballot(row.isu && lane < u && (fx >> lane & 1) && row.a == au));
            int cap = 0x7fffffff;
            if (cp) cap = cp[au];
            conflicts += (al && !al[u * M + au]) + (before >= (cap < 0 ? 0 : cap));
        }
#pragma unroll
        for (int j = 0; j < TPL; ++j) {
            const int t = lane + kWave * j;
            if (t >= M) continue;
            if (isfx) {
                if (au == t) {
                    may[j] |= 1u << u;
                    must[j] |= 1u << u;
                }
            } else if (!al || al[u * M + t]) {
                may[j] |= 1u << u;
            }
        }
    }
    ExactMask* mk = reinterpret_cast<ExactMask*>(ws + (long long)r * row_bytes + mask_off);
#pragma unroll
    for (int j = 0; j < TPL; ++j) {
        const int t = lane + kWave * j;
        if (t >= M) continue;
        int cap = N;
        if (cp) cap = cp[t] < 0 ? 0 : cp[t];
        const int held = __popc(must[j]);
        ExactMask m;
        m.may = (uint16_t)may[j];
        m.must = (uint16_t)must[j];
        m.cap = cap > held ? cap : held;
        mk[t] = m;
    }
    if (stats && lane < 2) stats[(long long)s * 2 + lane] = lane == 0 ? row.invalid : conflicts;
}

// ------------------------------------------------------------------ one stage
__global__ __launch_bounds__(kWave) void k_exact_stage(uavhip_env env, int stride, int s0, int t, int first,
                                                       char* __restrict__ ws, long long row_bytes, long long d_bytes,
                                                       long long choice_off, long long mask_off) {
    __shared__ double tile[kExactTile], comb[kExactTile], accv[kExactTile];
    __shared__ uint16_t accc[kExactTile];
    const int N = env.N, M = env.M, lane = threadIdx.x;
    const int L = N < kExactLowBits ? N : kExactLowBits, H = N - L, nl = 1 << L;
    const int r = blockIdx.x >> H;
    const unsigned Sh = blockIdx.x & ((1u << H) - 1);
    char* rw = ws + (long long)r * row_bytes;
    const double* dprev = reinterpret_cast<const double*>(rw + (long long)(t & 1) * d_bytes);
    double* dnext = reinterpret_cast<double*>(rw + (long long)((t + 1) & 1) * d_bytes);
    uint16_t* choice = reinterpret_cast<uint16_t*>(rw + choice_off) + ((long long)t << N);
    const ExactMask mk = reinterpret_cast<const ExactMask*>(rw + mask_off)[t];
    const double ninf = -__builtin_huge_val();

    // lane u: 1 - P[u][t] and omega c[u] of the row's active scene
    const long long e = (long long)(s0 + r) * stride;
    const long long sb =
        (env.scene_buffers == 2 ? (long long)(env.istate[e * UAVHIP_IST_COUNT + UAVHIP_IST_SCENE_SEL] & 1) * env.E : 0) + e;
    const double v = env.tgt_value[sb * M + t];
    double om = 1.0, wc = 0.0;
    if (lane < N) {
        om = 1.0 - env.p_dmg[(sb * N + lane) * M + t] * env.p_pen[sb * N + lane];
        wc = env.prm[UAVHIP_PRM_OMEGA] * env.uav_cost[sb * N + lane];
    }

    const unsigned lo = nl - 1;
    const unsigned mayl = mk.may & lo, mustl = mk.must & lo, mayh = mk.may >> L, musth = mk.must >> L;
    for (int i = lane; i < nl; i += kWave) {
        accv[i] = ninf;
        accc[i] = 0;
    }
    // the lane's share of ql / cl: the low six bits of a tile index lane + 64 k are the lane's
    double qlane = 1.0, clane = 0.0;
    for (int b = 0; b < (L < 6 ? L : 6); ++b) {
        const double ob = readlane_d(om, b), cb = readlane_d(wc, b);
        if (lane >> b & 1) {
            qlane = qlane * ob;
            clane = clane + cb;
        }
    }
    const uint16_t *off, *list;
    exact_sched(L, off, list);
    const int k0 = off[lane], k1 = off[lane + 1];

    if ((Sh & musth) == musth) {  // else no feasible T for any state of the tile: every D stays -inf
        const unsigned Eh = Sh & mayh & ~musth;
        unsigned Xh = Eh;
        for (;;) {
            const unsigned Th = musth | Xh;
            const int nh = __popc(Th);
            if (nh <= mk.cap) {
                double qh = 1.0, chs = 0.0;
                for (int b = 0; b < H; ++b)
                    if (Th >> b & 1) {
                        qh = qh * readlane_d(om, L + b);
                        chs = chs + readlane_d(wc, L + b);
                    }
                const double A = v - chs, B = v * qh;
                const double* src = dprev + ((long long)(Sh ^ Th) << L);
                __syncthreads();  // the previous Th's readers are done with tile / comb
                for (int k = 0; (k << 6) < nl; ++k) {
                    const int i = lane + (k << 6);
                    if (i >= nl) break;
                    tile[i] = first ? 0.0 : src[i];
                    double qk = 1.0, ck = 0.0;
                    for (int b = 6; b < L; ++b)
                        if (k >> (b - 6) & 1) {
                            qk = qk * readlane_d(om, b);
                            ck = ck + readlane_d(wc, b);
                        }
                    const double val = (A - (clane + ck)) - B * (qlane * qk);
                    comb[i] = nh + __popc(i) <= mk.cap ? val : ninf;
                }
                __syncthreads();

                // the flattened walk over the lane's states
                int k = k0;
                bool active = false;
                unsigned S = 0, E = 0, X = 0;
                double best = ninf;
                unsigned bestT = 0;
                auto take = [&]() {  // the next state of the list whose low part holds the fixed UAVs
                    active = false;
                    while (k < k1) {
                        S = list[k];
                        if ((S & mustl) == mustl) {
                            active = true;
                            E = S & mayl & ~mustl;
                            X = E;
                            best = accv[S];
                            bestT = accc[S];
                            break;
                        }
                        ++k;
                    }
                };
                take();
                while (active) {
                    const unsigned T = mustl | X;
                    const double cand = tile[S ^ T] + comb[T];
                    if (cand >= best) {  // descending T: of equal values the smallest T stays
                        best = cand;
                        bestT = Th << L | T;
                    }
                    if (X == 0) {
                        accv[S] = best;
                        accc[S] = (uint16_t)bestT;
                        ++k;
                        take();
                    } else {
                        X = (X - 1) & E;
                    }
                }
            }
            if (Xh == 0) break;
            Xh = (Xh - 1) & Eh;
        }
    }
    __syncthreads();
    double* dst = dnext + ((long long)Sh << L);
    uint16_t* cdst = choice + ((long long)Sh << L);
    for (int i = lane; i < nl; i += kWave) {
        dst[i] = accv[i];
        cdst[i] = accc[i];
    }
}

// ------------------------------------------------------------------ backtrack
template <int TPL, int NCAP>
__global__ __launch_bounds__(64 * kRefineWaves) void k_exact_backtrack(uavhip_env env, int stride, int s0, int R,
                                                                       const char* __restrict__ ws, long long row_bytes,
                                                                       long long choice_off, int* aout,
                                                                       double* __restrict__ J, int* __restrict__ covered) {
    const int r = blockIdx.x * kRefineWaves + (threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    if (r >= R) return;
    const int s = s0 + r;
    RefineRow<TPL, NCAP> row;
    row.load(env, s, stride, lane);
    row.load_columns();
    const int N = row.N;
    const uint16_t* choice = reinterpret_cast<const uint16_t*>(ws + (long long)r * row_bytes + choice_off);
    unsigned S = (1u << N) - 1;
    for (int t = row.M - 1; t >= 0; --t) {
        // T <= S by construction; the mask keeps the next index inside the table whatever the memory holds
        const unsigned T = (unsigned)__builtin_amdgcn_readfirstlane((int)choice[((long long)t << N) + S]) & S;
        if (lane < N && (T >> lane & 1)) row.a = t;
        S &= ~T;
    }
    row.finish(s, aout, J, covered);
}

}  // namespace
}  // namespace uavhip

extern "C" int64_t uavhip_exact_workspace_bytes(int32_t N, int32_t M, int32_t rows) {
    if (N < 1 || N > UAVHIP_EXACT_MAX_N || M < 1 || M > UAVHIP_MAX_M || rows < 1) return -1;
    return uavhip::exact_layout(N, M).row_bytes * rows;
}

extern "C" int uavhip_solve_exact(const uavhip_env* env, int32_t env_stride, int32_t S, const uint8_t* allowed,
                                  const uint8_t* fixed, const int32_t* capacity, const int32_t* assignment_in,
                                  int32_t* assignment_out, double* J, int32_t* covered, int32_t* stats, void* workspace,
                                  int64_t workspace_bytes, uavhip_stream_t stream) {
    using namespace uavhip;
    const char* fn = "uavhip_solve_exact";
    if (const int rc = check_rows(fn, env, env_stride, S, assignment_out && J && covered, "N <= %d",
                                  UAVHIP_EXACT_MAX_N))
        return rc;
    if (env->N > UAVHIP_EXACT_MAX_N) {
        set_error("%s: N=%d > UAVHIP_EXACT_MAX_N=%d (the choice table holds 16-bit sets and the DP takes 3^N steps a target)",
                  fn, env->N, UAVHIP_EXACT_MAX_N);
        return UAVHIP_EINVAL;
    }
    if (fixed && !assignment_in) {
        set_error("%s: fixed without assignment_in (a fixed UAV keeps the target assignment_in gives it)", fn);
        return UAVHIP_EINVAL;
    }
    const ExactLayout w = exact_layout(env->N, env->M);
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < w.row_bytes) {
        set_error("%s: workspace=%p (16-byte aligned) of %lld bytes holds no row: one row of %d x %d needs %lld "
                  "(uavhip_exact_workspace_bytes)", fn, workspace, (long long)workspace_bytes, env->N, env->M,
                  w.row_bytes);
        return UAVHIP_EINVAL;
    }
    const long long fit = workspace_bytes / w.row_bytes;
    const int chunk = (int)(fit < S ? fit : S);
    const int H = env->N > kExactLowBits ? env->N - kExactLowBits : 0;
    char* ws = static_cast<char*>(workspace);
    for (int s0 = 0; s0 < S; s0 += chunk) {
        const int R = S - s0 < chunk ? S - s0 : chunk;
        UAVHIP_ROWS_LAUNCH(env, R, (k_exact_prepare<TPL, NCAP>), stream, *env, (int)env_stride, s0, R, allowed, fixed,
                           capacity, assignment_in, ws, w.row_bytes, w.mask_off, stats);
        for (int t = 0; t < env->M; ++t)
            hipLaunchKernelGGL(k_exact_stage, dim3((unsigned)R << H), dim3(kWave), 0, (hipStream_t)stream, *env,
                               (int)env_stride, s0, t, (int)(t == 0), ws, w.row_bytes, w.d_bytes, w.choice_off, w.mask_off);
        UAVHIP_ROWS_LAUNCH(env, R, (k_exact_backtrack<TPL, NCAP>), stream, *env, (int)env_stride, s0, R, ws, w.row_bytes,
                           w.choice_off, assignment_out, J, covered);
        if (const int rc = check_launch("k_exact_stage")) return rc;
    }
    return UAVHIP_OK;
}
