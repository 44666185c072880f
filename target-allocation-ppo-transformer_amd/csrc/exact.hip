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
// A stage's tile (exact_stage_tile, exact_device.hpp: shared with exact_free.hip): the UAV bits split into L = min(N, 10) low and H = N - L high bits, and one wave
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
#include "exact_device.hpp"

namespace uavhip {
namespace {

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
    const int N = env.N, M = env.M, lane = threadIdx.x;
    const int L = N < kExactLowBits ? N : kExactLowBits, H = N - L;
    const int r = blockIdx.x >> H;
    const unsigned Sh = blockIdx.x & ((1u << H) - 1);
    char* rw = ws + (long long)r * row_bytes;
    const double* dprev = reinterpret_cast<const double*>(rw + (long long)(t & 1) * d_bytes);
    double* dnext = reinterpret_cast<double*>(rw + (long long)((t + 1) & 1) * d_bytes);
    uint16_t* choice = reinterpret_cast<uint16_t*>(rw + choice_off) + ((long long)t << N);
    const ExactMask mk = reinterpret_cast<const ExactMask*>(rw + mask_off)[t];

    // lane u: 1 - P[u][t] and omega c[u] of the row's active scene
    const long long sb = row_scene_base(env, s0 + r, stride);
    const double v = env.tgt_value[sb * M + t];
    double om = 1.0, wc = 0.0;
    if (lane < N) {
        om = 1.0 - env.p_dmg[(sb * N + lane) * M + t] * env.p_pen[sb * N + lane];
        wc = env.prm[UAVHIP_PRM_OMEGA] * env.uav_cost[sb * N + lane];
    }

    exact_stage_tile(N, Sh, first, v, om, wc, mk, dprev, dnext, choice);
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
    if (const int rc = check_dp_workspace(fn, workspace, workspace_bytes, w.row_bytes, "uavhip_exact_workspace_bytes",
                                          "%d x %d", env->N, env->M))
        return rc;
    const int H = env->N > kExactLowBits ? env->N - kExactLowBits : 0;
    char* ws = static_cast<char*>(workspace);
    return for_row_chunks(S, workspace_bytes / w.row_bytes, [&](int s0, int R) {
        UAVHIP_ROWS_LAUNCH(env, R, (k_exact_prepare<TPL, NCAP>), stream, *env, (int)env_stride, s0, R, allowed, fixed,
                           capacity, assignment_in, ws, w.row_bytes, w.mask_off, stats);
        for (int t = 0; t < env->M; ++t)
            hipLaunchKernelGGL(k_exact_stage, dim3((unsigned)R << H), dim3(kWave), 0, (hipStream_t)stream, *env,
                               (int)env_stride, s0, t, (int)(t == 0), ws, w.row_bytes, w.d_bytes, w.choice_off, w.mask_off);
        UAVHIP_ROWS_LAUNCH(env, R, (k_exact_backtrack<TPL, NCAP>), stream, *env, (int)env_stride, s0, R, ws, w.row_bytes,
                           w.choice_off, assignment_out, J, covered);
        return check_launch("k_exact_stage");
    });
}
