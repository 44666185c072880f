// refine_device.hpp -- the device side of the best-response local search on J(X), shared by k_refine
// (refine.hip, uavhip_refine_assignments), k_search (search.hip, uavhip_search_assignments) and
// k_search_constrained (search_constrained.hip, uavhip_search_assignments_constrained): one wave's
// view of one row -- the scene's registers, the id conversion, the sweeps and the scoring of the
// result. All three translation units are built with -ffp-contract=off; the rule is in
// include/uavhip.h.
//
// One wave per row. Lane t owns target t (and t + 64 when M > 64): its value, its id and the running
// product Q; lane u owns a[u], p_pen[u] and omega c[u]. Q[t] is rebuilt for every UAV as the
// ascending product over the other UAVs on t -- never kept incrementally, its rounding would depend
// on the history of moves:
//  * NCAP > 0 (M <= 64, N <= NCAP <= 32): lane t holds the column 1 - P[w][t], w < N, in registers
//    and the rebuild is N readlanes of a[w] and a predicated multiply each: no memory access;
//  * NCAP == 0 (N > 32 or M > 64): only the assigned UAVs contribute, so the rebuild loads the one
//    element p_dmg[w][a[w]] per assigned w (L1 / L2 hits after the first sweep) in lane a[w].
#pragma once
#include <cstdarg>
#include <cstdio>

#include "common.hpp"

namespace uavhip {

constexpr int kRefineWaves = 4;

// maximum of (g, t) over the wave, the lowest t among equal g; every lane gets the result
__device__ __forceinline__ void wave_argmax(double& g, int& t) {
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        const double go = __shfl_xor(g, m);
        const int to = __shfl_xor(t, m);
        if (go > g || (go == g && to < t)) {
            g = go;
            t = to;
        }
    }
}
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) x = x + __shfl_xor(x, m);
    return x;
}

// element base of the active scene of the row's env, s * stride: buffer istate[SCENE_SEL] (env_device.hpp)
__device__ __forceinline__ long long row_scene_base(const uavhip_env& env, int s, int stride) {
    const long long e = (long long)s * stride;
    return (env.scene_buffers == 2 ? (long long)(env.istate[e * UAVHIP_IST_COUNT + UAVHIP_IST_SCENE_SEL] & 1) * env.E : 0) + e;
}

// word `index` & 3 of the Philox4x32-10 block of counter {index >> 2, round, s, stream}
__device__ __forceinline__ uint32_t philox_word(uint32_t index, uint32_t round, uint32_t s, uint32_t stream,
                                                uint32_t key0, uint32_t key1) {
    const u32x4 x = philox(u32x4{index >> 2, round, s, stream}, key0, key1);
    return (index & 2) ? ((index & 1) ? x.w : x.z) : ((index & 1) ? x.y : x.x);
}

// What uavhip_search_assignments_constrained adds to a row (LIM): lane t holds, per target slot, the
// UAVs that may take it and its capacity; `fixed` is wave-uniform. RefineRow's default holds nothing
// and its sweeps are the unconstrained ones, instruction for instruction.
template <int TPL, bool LIM>
struct RowLimits {};
template <int TPL>
struct RowLimits<TPL, true> {
    unsigned long long ok[TPL];  // bit u: allowed[u][t] of the lane's targets
    int cap[TPL];                // capacity[t] of the lane's targets, >= 0
    unsigned long long fixed;    // bit u: UAV u is fixed
};

template <int TPL, int NCAP, bool LIM = false>
struct RefineRow {
    static_assert(NCAP == 0 || TPL == 1, "the register column is the one-target-per-lane path");
    int N, M, lane;
    double omega;
    const double* __restrict__ pd;  // p_dmg of the row's active scene, [N][M]
    double v[TPL];                  // tgt_value of the lane's targets (0.0 beyond M)
    int id[TPL];                    // tgt_id of the lane's targets
    bool isu;
    double pen, cost, wc;           // p_pen[lane], uav_cost[lane], omega * uav_cost[lane]
    int a, invalid;                 // a[lane]: list index or -1; ids of the input that matched nothing
    double om[NCAP > 0 ? NCAP : 1];
    int sweeps, moves, converged;
    RowLimits<TPL, LIM> lim;

    // the scene of env s * stride (its active buffer) into registers; every UAV at -1
    __device__ __forceinline__ void load(const uavhip_env& env, int s, int stride, int lane_) {
        N = env.N;
        M = env.M;
        lane = lane_;
        const long long sb = row_scene_base(env, s, stride);
        omega = env.prm[UAVHIP_PRM_OMEGA];
        pd = env.p_dmg + sb * N * M;
#pragma unroll
        for (int j = 0; j < TPL; ++j) {
            const int t = lane + kWave * j;
            v[j] = t < M ? env.tgt_value[sb * M + t] : 0.0;
            id[j] = t < M ? env.tgt_id[sb * M + t] : 0;
        }
        isu = lane < N;
        pen = isu ? env.p_pen[sb * N + lane] : 0.0;
        cost = isu ? env.uav_cost[sb * N + lane] : 0.0;
        wc = omega * cost;
        a = -1;
        invalid = 0;
        sweeps = 0;
        moves = 0;
        converged = 1;
    }

    // target ids -> list indices: a ballot against the lanes' ids, the lowest list index first
    __device__ __forceinline__ void convert(const int* ain, int s) {
        if (!ain) return;
        const int idin = isu ? ain[(long long)s * N + lane] : -1;
        for (int u = 0; u < N; ++u) {
            const int want = readlane_i(idin, u);
            if (want == -1) continue;
            int idx = -1;
#pragma unroll
            for (int j = TPL - 1; j >= 0; --j) {
                const unsigned long long m = ballot(lane + kWave * j < M && id[j] == want);
                if (m) idx = kWave * j + ffs64(m);
            }
            if (idx < 0) ++invalid;
            if (lane == u) a = idx;
        }
    }

    __device__ __forceinline__ void load_columns() {
        if constexpr (NCAP > 0) {
#pragma unroll
            for (int w = 0; w < NCAP; ++w) {
                om[w] = 1.0;
                if (w < N) {
                    const double pw = readlane_d(pen, w);
                    if (lane < M) om[w] = 1.0 - pd[w * M + lane] * pw;
                }
            }
        }
    }

    // Q[j] = product of (1 - P[w][t]) over w != skip with a[w] == t, ascending w, from 1.0;
    // cnt[j] = the number of those w
    __device__ __forceinline__ void build_q(int skip, double (&Q)[TPL], int (&cnt)[TPL]) const {
#pragma unroll
        for (int j = 0; j < TPL; ++j) {
            Q[j] = 1.0;
            cnt[j] = 0;
        }
        if constexpr (NCAP > 0) {
#pragma unroll
            for (int w = 0; w < NCAP; ++w) {
                if (w < N) {
                    const int aw = readlane_i(a, w);
                    if (aw == lane && w != skip) {
                        Q[0] = Q[0] * om[w];
                        ++cnt[0];
                    }
                }
            }
        } else {
            for (int w = 0; w < N; ++w) {
                const int aw = readlane_i(a, w);
                if (aw < 0 || w == skip) continue;
                const double pw = readlane_d(pen, w);
#pragma unroll
                for (int j = 0; j < TPL; ++j) {
                    if (aw == lane + kWave * j) {
                        Q[j] = Q[j] * (1.0 - pd[w * M + aw] * pw);
                        ++cnt[j];
                    }
                }
            }
        }
    }

    // best-response sweeps from a, until a sweep makes no move or max_sweeps sweeps of this call
    // have run; sweeps and moves accumulate over calls, converged is this call's. With LIM a fixed
    // UAV is not visited, and a free one chooses among the targets it may take that have room
    // (cnt, the other UAVs on t, < cap) or are its own.
    __device__ __forceinline__ void phase(int max_sweeps) {
        const long long last = (long long)sweeps + max_sweeps;
        converged = 1;
        while (sweeps < last) {
            int moved = 0;
            for (int u = 0; u < N; ++u) {
                int own = -1;
                if constexpr (LIM) {
                    if (lim.fixed >> u & 1) continue;
                    own = readlane_i(a, u);
                }
                double Q[TPL];
                int cnt[TPL];
                build_q(u, Q, cnt);
                const double pu = readlane_d(pen, u), wcu = readlane_d(wc, u);
                double g[TPL];
                double bg = -__builtin_huge_val();
                int bt = 0x7fffffff;
#pragma unroll
                for (int j = 0; j < TPL; ++j) {
                    const int t = lane + kWave * j;
                    g[j] = -__builtin_huge_val();
                    if (t < M) {
                        const double p = pd[u * M + t] * pu;
                        g[j] = (v[j] * Q[j]) * p - wcu;
                        bool may = true;
                        if constexpr (LIM) may = (lim.ok[j] >> u & 1) && (t == own || cnt[j] < lim.cap[j]);
                        if (may && g[j] > bg) {
                            bg = g[j];
                            bt = t;
                        }
                    }
                }
                wave_argmax(bg, bt);
                bg = readlane_d(bg, 0);
                bt = readlane_i(bt, 0);
                const int au = readlane_i(a, u);
                double cur = 0.0;
                if (au >= 0) {
                    if constexpr (TPL == 2)
                        cur = readlane_d(au >= kWave ? g[1] : g[0], au & (kWave - 1));
                    else
                        cur = readlane_d(g[0], au);
                }
                const bool some = bg > 0.0;
                const int cand = some ? bt : -1;
                const double cg = some ? bg : 0.0;
                if (cg > cur) {
                    if (lane == u) a = cand;
                    ++moves;
                    moved = 1;
                }
            }
            ++sweeps;
            converged = !moved;
            if (!moved) break;
        }
    }

    // J and covered of a, and a as target ids
    __device__ __forceinline__ void finish(int s, int* aout, double* __restrict__ J, int* __restrict__ covered) const {
        double Q[TPL];
        int cnt[TPL];
        build_q(-1, Q, cnt);
        double val = 0.0;
        int cov = 0;
#pragma unroll
        for (int j = 0; j < TPL; ++j) {
            val = val + v[j] * (1.0 - Q[j]);  // v = 0 beyond M
            cov += __popcll(ballot(cnt[j] > 0));
        }
        val = wave_sum(val);
        const double csum = wave_sum(a >= 0 ? cost : 0.0);
        const int src = a < 0 ? 0 : a;
        int out = __shfl(id[0], src & (kWave - 1));
        if constexpr (TPL == 2) {
            const int hi = __shfl(id[1], src & (kWave - 1));
            out = src >= kWave ? hi : out;
        }
        if (isu) aout[(long long)s * N + lane] = a < 0 ? -1 : out;
        if (lane == 0) {
            J[s] = val - omega * csum;
            covered[s] = cov;
        }
    }
};

// ------------------------------------------------------------------ host: what the entry points share
// The env and the rows of entry point `fn` (row s < S on the scene of env s * env_stride), and the rest
// of its arguments: `rest_ok`, with `caps` (a format and its values) naming the caps in the message.
inline int check_rows(const char* fn, const uavhip_env* env, int32_t env_stride, int32_t S, bool rest_ok,
                      const char* caps, ...) {
    if (const int rc = validate_env_for(fn, env, false)) return rc;
    if (env_stride >= 1 && S >= 1 && (long long)(S - 1) * env_stride < env->E && rest_ok) return UAVHIP_OK;
    char c[96];
    va_list ap;
    va_start(ap, caps);
    vsnprintf(c, sizeof c, caps, ap);
    va_end(ap);
    set_error("%s: need env_stride=%d >= 1, S=%d >= 1, (S - 1) * env_stride < E=%d, %s and assignment_out/J/covered "
              "non-NULL", fn, env_stride, S, env->E, c);
    return UAVHIP_EINVAL;
}

}  // namespace uavhip

// UAVHIP_WITH_ROW_SHAPE runs its statement with RefineRow's TPL and NCAP bound to the constants of the
// env's shape: two targets per lane for M > 64, else the register column of the smallest cap that holds
// N. UAVHIP_ROWS_LAUNCH launches `kern` (an expression in them, in parentheses) over S rows, one wave each.
#define UAVHIP_ROWS_CASE(T, C, ...)      \
    {                                    \
        constexpr int TPL = T, NCAP = C; \
        __VA_ARGS__;                     \
    }
#define UAVHIP_WITH_ROW_SHAPE(env, ...)                                          \
    do {                                                                         \
        if ((env)->M > ::uavhip::kWave) UAVHIP_ROWS_CASE(2, 0, __VA_ARGS__)      \
        else if ((env)->N <= 8) UAVHIP_ROWS_CASE(1, 8, __VA_ARGS__)              \
        else if ((env)->N <= 16) UAVHIP_ROWS_CASE(1, 16, __VA_ARGS__)            \
        else if ((env)->N <= 32) UAVHIP_ROWS_CASE(1, 32, __VA_ARGS__)            \
        else UAVHIP_ROWS_CASE(1, 0, __VA_ARGS__)                                 \
    } while (0)
#define UAVHIP_ROWS_LAUNCH(env, S, kern, stream, ...)                                                              \
    UAVHIP_WITH_ROW_SHAPE(env, hipLaunchKernelGGL(kern, dim3(((S) + ::uavhip::kRefineWaves - 1) / ::uavhip::kRefineWaves), \
                                                  dim3(64 * ::uavhip::kRefineWaves), 0, (hipStream_t)(stream), __VA_ARGS__))
