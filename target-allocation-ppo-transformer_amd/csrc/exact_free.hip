// exact_free.hip -- the optimum of J(X) over the assignments of a row's FREE UAVs, everyone else held
// where the input puts them (uavhip_solve_exact_free), for the full N <= 64, M <= 128; and the choice of
// a round's free set on device (uavhip_neighbourhood_pick). The rules are in include/uavhip.h. Built
// with -ffp-contract=off: the stage is exact.hip's own (exact_device.hpp), and J, covered and the ids of
// the result come from RefineRow::finish.
//
// The subset DP runs over K = min(max_free, N) bits, bit b the b-th free UAV of the row in ascending
// order. A held UAV (fixed, or free beyond the first K) changes only the value of its target:
//   val_t(T_held + T) - val_t(T_held) = (v[t] q_fix[t]) (1 - prod_{u in T} (1 - P[u][t])) - w sum_{u in T} c[u]
// with q_fix[t] the product of 1 - P[u][t] over the held UAVs on t, so a stage is exact.hip's with
// v[t] q_fix[t] for v[t], no `must` set, and the capacity the held UAVs leave. A row with fewer than K
// free UAVs runs the same tables with dead bits: no target may hold them, their lanes carry 1.0 and 0.0,
// and the live bits are the lowest, so the tile's arithmetic is that of a table of the live bits alone.
//
// Three kernels per chunk of rows, as exact.hip's, stream-ordered on one workspace:
//   k_exact_free_prepare    one wave per row: the id conversion, the free list, per target its record
//                           (the bits that may take it, the capacity left, v q_fix) and stats;
//   k_exact_free_stage      one launch per target: exact_stage_tile on the row's free list;
//   k_exact_free_backtrack  one wave per row: the held UAVs where they came from, the free ones where
//                           choice_t puts them from t = M-1 down, then finish.
// Row workspace: D_t, D_{t+1} [2^K] f64 | choice [M][2^K] u16 | records [M] of 16 bytes | free list [16] u8.
#include "exact_device.hpp"

namespace uavhip {
namespace {

constexpr int kFreeMax = UAVHIP_EXACT_FREE_MAX;

struct FreeTarget {
    ExactMask mk;  // may: the free-list bits allowed on the target; must = 0; cap: what the held UAVs leave
    double vq;     // v[t] q_fix[t]
};
static_assert(sizeof(FreeTarget) == 16, "the row layout counts 16 bytes a target");

struct FreeLayout {
    long long d_bytes, choice_off, tgt_off, list_off, row_bytes;
};
inline FreeLayout free_layout(int K, int M) {
    FreeLayout w;
    w.d_bytes = (long long)sizeof(double) << K;
    w.choice_off = 2 * w.d_bytes;
    w.tgt_off = (w.choice_off + ((long long)M * (long long)sizeof(uint16_t) << K) + 15) & ~15ll;
    w.list_off = w.tgt_off + (long long)M * (long long)sizeof(FreeTarget);
    w.row_bytes = w.list_off + kFreeMax;
    return w;
}

// The row's sets as 64-bit masks over the UAVs: `dp` the free UAVs in the DP (the first K with
// fixed == 0, ascending), `held` every other UAV.
struct FreeSets {
    unsigned long long dp, held;
    int overflow;  // free UAVs beyond the first K
};
template <class Row>
__device__ __forceinline__ FreeSets free_sets(const Row& row, const uint8_t* fixed, int s, int K) {
    const unsigned long long all = ballot(row.isu);
    const unsigned long long fx = ballot(fixed && row.isu && fixed[(long long)s * row.N + row.lane]);
    unsigned long long rest = all & ~fx;
    FreeSets f;
    f.dp = 0;
    for (int b = 0; b < K && rest; ++b) {
        f.dp |= rest & (~rest + 1);
        rest &= rest - 1;
    }
    f.held = all & ~f.dp;
    f.overflow = __popcll(rest);
    return f;
}

// ------------------------------------------------------------------ prepare
template <int TPL, int NCAP>
__global__ __launch_bounds__(64 * kRefineWaves) void k_exact_free_prepare(
    uavhip_env env, int stride, int s0, int R, int K, const uint8_t* __restrict__ allowed,
    const uint8_t* __restrict__ fixed, const int* __restrict__ capacity, const int* ain, char* __restrict__ ws,
    long long row_bytes, long long tgt_off, long long list_off, int* __restrict__ stats) {
    const int r = blockIdx.x * kRefineWaves + (threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    if (r >= R) return;
    const int s = s0 + r;
    RefineRow<TPL, NCAP> row;
    row.load(env, s, stride, lane);
    row.convert(ain, s);
    const int N = row.N, M = row.M;
    const FreeSets f = free_sets(row, fixed, s, K);
    const uint8_t* al = allowed ? allowed + (long long)s * N * M : nullptr;
    const int* cp = capacity ? capacity + (long long)s * M : nullptr;

    int conflicts = 0, bit = 0;
    unsigned may[TPL];
    int heldn[TPL];
    double q[TPL];
#pragma unroll
    for (int j = 0; j < TPL; ++j) {
        may[j] = 0;
        heldn[j] = 0;
        q[j] = 1.0;
    }
    for (int u = 0; u < N; ++u) {
        const int au = readlane_i(row.a, u);
        if (f.held >> u & 1) {
            if (au < 0) continue;
            // the held UAVs below u on the same target: n[a[u]] of pass 1
            const int before = __popcll(ballot(row.isu && lane < u && (f.held >> lane & 1) && row.a == au));
            int cap = 0x7fffffff;
            if (cp) cap = cp[au];
            conflicts += (al && !al[u * M + au]) + (before >= (cap < 0 ? 0 : cap));
            const double pu = readlane_d(row.pen, u);
#pragma unroll
            for (int j = 0; j < TPL; ++j)
                if (au == lane + kWave * j) {
                    q[j] = q[j] * (1.0 - row.pd[u * M + au] * pu);
                    ++heldn[j];
                }
        } else {
#pragma unroll
            for (int j = 0; j < TPL; ++j) {
                const int t = lane + kWave * j;
                if (t < M && (!al || al[u * M + t])) may[j] |= 1u << bit;
            }
            ++bit;
        }
    }
    char* rw = ws + (long long)r * row_bytes;
    FreeTarget* tg = reinterpret_cast<FreeTarget*>(rw + tgt_off);
#pragma unroll
    for (int j = 0; j < TPL; ++j) {
        const int t = lane + kWave * j;
        if (t >= M) continue;
        int cap = N;
        if (cp) cap = cp[t] < 0 ? 0 : cp[t];
        FreeTarget m;
        m.mk.may = (uint16_t)may[j];
        m.mk.must = 0;
        m.mk.cap = (cap > heldn[j] ? cap : heldn[j]) - heldn[j];
        m.vq = row.v[j] * q[j];
        tg[t] = m;
    }
    // the free list: lane b < 16 holds the UAV of bit b, 0xFF for a dead bit
    if (lane < kFreeMax) {
        unsigned long long rest = f.dp;
        for (int b = 0; b < lane; ++b) rest &= rest - 1;
        reinterpret_cast<uint8_t*>(rw + list_off)[lane] = rest ? (uint8_t)ffs64(rest) : (uint8_t)0xFF;
    }
    if (stats && lane < 4)
        stats[(long long)s * 4 + lane] =
            lane == 0 ? row.invalid : lane == 1 ? conflicts : lane == 2 ? __popcll(f.dp) : f.overflow;
}

// ------------------------------------------------------------------ one stage
__global__ __launch_bounds__(kWave) void k_exact_free_stage(uavhip_env env, int stride, int s0, int K, int t, int first,
                                                            char* __restrict__ ws, long long row_bytes,
                                                            long long d_bytes, long long choice_off, long long tgt_off,
                                                            long long list_off) {
    const int N = env.N, M = env.M, lane = threadIdx.x;
    const int L = K < kExactLowBits ? K : kExactLowBits, H = K - L;
    const int r = blockIdx.x >> H;
    const unsigned Sh = blockIdx.x & ((1u << H) - 1);
    char* rw = ws + (long long)r * row_bytes;
    const double* dprev = reinterpret_cast<const double*>(rw + (long long)(t & 1) * d_bytes);
    double* dnext = reinterpret_cast<double*>(rw + (long long)((t + 1) & 1) * d_bytes);
    uint16_t* choice = reinterpret_cast<uint16_t*>(rw + choice_off) + ((long long)t << K);
    const FreeTarget tg = reinterpret_cast<const FreeTarget*>(rw + tgt_off)[t];

    // lane b: 1 - P[u][t] and omega c[u] of the UAV u of bit b; 1.0 and 0.0 for a dead bit
    const long long sb = row_scene_base(env, s0 + r, stride);
    double om = 1.0, wc = 0.0;
    if (lane < K) {
        const int u = reinterpret_cast<const uint8_t*>(rw + list_off)[lane];
        if (u < N) {
            om = 1.0 - env.p_dmg[(sb * N + u) * M + t] * env.p_pen[sb * N + u];
            wc = env.prm[UAVHIP_PRM_OMEGA] * env.uav_cost[sb * N + u];
        }
    }
    exact_stage_tile(K, Sh, first, tg.vq, om, wc, tg.mk, dprev, dnext, choice);
}

// ------------------------------------------------------------------ backtrack
template <int TPL, int NCAP>
__global__ __launch_bounds__(64 * kRefineWaves) void k_exact_free_backtrack(
    uavhip_env env, int stride, int s0, int R, int K, const uint8_t* __restrict__ fixed, const int* ain,
    const char* __restrict__ ws, long long row_bytes, long long choice_off, int* aout, double* __restrict__ J,
    int* __restrict__ covered) {
    const int r = blockIdx.x * kRefineWaves + (threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    if (r >= R) return;
    const int s = s0 + r;
    RefineRow<TPL, NCAP> row;
    row.load(env, s, stride, lane);
    row.convert(ain, s);
    row.load_columns();
    const FreeSets f = free_sets(row, fixed, s, K);
    // the lane's bit of the DP's sets, -1 for a held UAV; a free UAV starts on none
    const bool mine = f.dp >> lane & 1;
    const int bit = mine ? __popcll(f.dp & ((1ull << lane) - 1)) : -1;
    if (mine) row.a = -1;
    const uint16_t* choice = reinterpret_cast<const uint16_t*>(ws + (long long)r * row_bytes + choice_off);
    unsigned S = (1u << K) - 1;
    for (int t = row.M - 1; t >= 0; --t) {
        // T <= S by construction; the mask keeps the next index inside the table whatever the memory holds
        const unsigned T = (unsigned)__builtin_amdgcn_readfirstlane((int)choice[((long long)t << K) + S]) & S;
        if (mine && (T >> bit & 1)) row.a = t;
        S &= ~T;
    }
    row.finish(s, aout, J, covered);
}

// ------------------------------------------------------------------ the neighbourhood of a round
// One wave per row. Lane u holds UAV u's key, lane t (and t + 64) the targets' keys; a rank is a count
// over readlanes, so nothing is sorted in memory. The keys are philox_word's (refine_device.hpp).
template <int TPL>
__global__ __launch_bounds__(64 * kRefineWaves) void k_neighbourhood_pick(
    uavhip_env env, int stride, int S, int K, int mode, uint32_t round, uint32_t key0, uint32_t key1, const int* ain,
    const uint8_t* __restrict__ fixed_in, uint8_t* __restrict__ fixed_out) {
    const int s = blockIdx.x * kRefineWaves + (threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    if (s >= S) return;
    RefineRow<TPL, 0> row;
    row.load(env, s, stride, lane);
    const int N = row.N, M = row.M;
    const bool open = row.isu && !(fixed_in && fixed_in[(long long)s * N + lane]);
    const uint32_t ku = philox_word((uint32_t)lane, round, (uint32_t)s, 0x4E424855u, key0, key1);
    uint32_t g = 0;
    if (mode == UAVHIP_NBH_TARGETS) {
        row.convert(ain, s);
        uint32_t kt[TPL];
        int rank[TPL];
#pragma unroll
        for (int j = 0; j < TPL; ++j) {
            kt[j] = philox_word((uint32_t)(lane + kWave * j), round, (uint32_t)s, 0x4E424854u, key0, key1);
            rank[j] = 0;
        }
        for (int t = 0; t < M; ++t) {
            const uint32_t other = TPL == 2 && t >= kWave ? readlane_u(kt[TPL - 1], t - kWave) : readlane_u(kt[0], t);
#pragma unroll
            for (int j = 0; j < TPL; ++j) {
                const int mine = lane + kWave * j;
                rank[j] += other < kt[j] || (other == kt[j] && t < mine);
            }
        }
        const int src = row.a < 0 ? 0 : row.a;
        int ra = __shfl(rank[0], src & (kWave - 1));
        if constexpr (TPL == 2) {
            const int hi = __shfl(rank[1], src & (kWave - 1));
            ra = src >= kWave ? hi : ra;
        }
        g = row.a < 0 ? 0u : 1u + (uint32_t)ra;
    }
    // the UAV's place among the open ones by (g, ku, u)
    int place = 0;
    const unsigned long long opens = ballot(open);
    for (int w = 0; w < N; ++w) {
        const uint32_t gw = readlane_u(g, w), kw = readlane_u(ku, w);
        const bool ow = opens >> w & 1;
        place += ow && (gw < g || (gw == g && (kw < ku || (kw == ku && w < lane))));
    }
    if (row.isu) fixed_out[(long long)s * N + lane] = open && place < K ? 0 : 1;
}

}  // namespace
}  // namespace uavhip

extern "C" int64_t uavhip_exact_free_workspace_bytes(int32_t max_free, int32_t M, int32_t rows) {
    if (max_free < 1 || max_free > UAVHIP_EXACT_FREE_MAX || M < 1 || M > UAVHIP_MAX_M || rows < 1) return -1;
    return uavhip::free_layout(max_free, M).row_bytes * rows;
}

extern "C" int uavhip_solve_exact_free(const uavhip_env* env, int32_t env_stride, int32_t S, int32_t max_free,
                                       const uint8_t* allowed, const uint8_t* fixed, const int32_t* capacity,
                                       const int32_t* assignment_in, int32_t* assignment_out, double* J,
                                       int32_t* covered, int32_t* stats, void* workspace, int64_t workspace_bytes,
                                       uavhip_stream_t stream) {
    using namespace uavhip;
    const char* fn = "uavhip_solve_exact_free";
    if (const int rc = check_rows(fn, env, env_stride, S,
                                  max_free >= 1 && max_free <= UAVHIP_EXACT_FREE_MAX && assignment_out && J && covered,
                                  "1 <= max_free=%d <= %d", max_free, UAVHIP_EXACT_FREE_MAX))
        return rc;
    if (fixed && !assignment_in) {
        set_error("%s: fixed without assignment_in (a held UAV keeps the target assignment_in gives it)", fn);
        return UAVHIP_EINVAL;
    }
    const int K = max_free < env->N ? max_free : env->N;  // more bits than UAVs would all be dead
    const FreeLayout w = free_layout(K, env->M);
    if (const int rc = check_dp_workspace(fn, workspace, workspace_bytes, w.row_bytes,
                                          "uavhip_exact_free_workspace_bytes", "%d free UAVs x %d targets", K, env->M))
        return rc;
    const int H = K > kExactLowBits ? K - kExactLowBits : 0;
    char* ws = static_cast<char*>(workspace);
    return for_row_chunks(S, workspace_bytes / w.row_bytes, [&](int s0, int R) {
        UAVHIP_ROWS_LAUNCH(env, R, (k_exact_free_prepare<TPL, NCAP>), stream, *env, (int)env_stride, s0, R, K, allowed,
                           fixed, capacity, assignment_in, ws, w.row_bytes, w.tgt_off, w.list_off, stats);
        for (int t = 0; t < env->M; ++t)
            hipLaunchKernelGGL(k_exact_free_stage, dim3((unsigned)R << H), dim3(kWave), 0, (hipStream_t)stream, *env,
                               (int)env_stride, s0, K, t, (int)(t == 0), ws, w.row_bytes, w.d_bytes, w.choice_off,
                               w.tgt_off, w.list_off);
        UAVHIP_ROWS_LAUNCH(env, R, (k_exact_free_backtrack<TPL, NCAP>), stream, *env, (int)env_stride, s0, R, K, fixed,
                           assignment_in, ws, w.row_bytes, w.choice_off, assignment_out, J, covered);
        return check_launch("k_exact_free_stage");
    });
}

extern "C" int uavhip_neighbourhood_pick(const uavhip_env* env, int32_t env_stride, int32_t S, int32_t K, int32_t mode,
                                         uint32_t round, uint64_t seed, const int32_t* assignment,
                                         const uint8_t* fixed_in, uint8_t* fixed_out, uavhip_stream_t stream) {
    using namespace uavhip;
    const char* fn = "uavhip_neighbourhood_pick";
    if (const int rc = validate_env_for(fn, env, false)) return rc;
    if (env_stride < 1 || S < 1 || (long long)(S - 1) * env_stride >= env->E || K < 1 || K > UAVHIP_EXACT_FREE_MAX ||
        (mode != UAVHIP_NBH_RANDOM && mode != UAVHIP_NBH_TARGETS) || !fixed_out) {
        set_error("%s: need env_stride=%d >= 1, S=%d >= 1, (S - 1) * env_stride < E=%d, 1 <= K=%d <= %d, mode=%d in "
                  "{UAVHIP_NBH_RANDOM, UAVHIP_NBH_TARGETS} and fixed_out non-NULL", fn, env_stride, S, env->E, K,
                  UAVHIP_EXACT_FREE_MAX, mode);
        return UAVHIP_EINVAL;
    }
    const dim3 grid((S + kRefineWaves - 1) / kRefineWaves), block(64 * kRefineWaves);
    if (env->M > kWave)
        hipLaunchKernelGGL(k_neighbourhood_pick<2>, grid, block, 0, (hipStream_t)stream, *env, (int)env_stride, (int)S,
                           (int)K, (int)mode, round, (uint32_t)seed, (uint32_t)(seed >> 32), assignment, fixed_in,
                           fixed_out);
    else
        hipLaunchKernelGGL(k_neighbourhood_pick<1>, grid, block, 0, (hipStream_t)stream, *env, (int)env_stride, (int)S,
                           (int)K, (int)mode, round, (uint32_t)seed, (uint32_t)(seed >> 32), assignment, fixed_in,
                           fixed_out);
    return check_launch("k_neighbourhood_pick");
}
