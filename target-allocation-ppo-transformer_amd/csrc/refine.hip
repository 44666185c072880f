// refine.hip -- best-response local search on the objective J(X) itself (uavhip_refine_assignments):
// polish a decoded allocation, build a non-learned baseline from the empty one, or only score an
// assignment that did not come from the env. The env decides each assignment on r(X) in one pass of
// the pointer walk (uav_env.py:295-435) and never revisits a UAV; here every UAV in turn moves to the
// target (or to none) where its marginal contribution to J (_calc_J_X, uav_env.py:244-269), the
// others held fixed, is largest. Built with -ffp-contract=off: the tests compare assignments bit for
// bit with a numpy restatement of the rule (include/uavhip.h).
//
// One wave per scene, four per workgroup (as k_select_best). Lane t owns target t (and t + 64 when
// M > 64): its value, its id and the running product Q; lane u owns a[u], p_pen[u] and omega c[u].
// Q[t] is rebuilt for every UAV as the ascending product over the other UAVs on t -- never kept
// incrementally, its rounding would depend on the history of moves:
//  * NCAP > 0 (M <= 64, N <= NCAP <= 32): lane t holds the column 1 - P[w][t], w < N, in registers
//    and the rebuild is N readlanes of a[w] and a predicated multiply each: no memory access;
//  * NCAP == 0 (N > 32 or M > 64): only the assigned UAVs contribute, so the rebuild loads the one
//    element p_dmg[w][a[w]] per assigned w (L1 / L2 hits after the first sweep) in lane a[w].
// The env and the scene are only read.
#include <cstdio>

#include "common.hpp"

namespace uavhip {
namespace {

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

template <int TPL, int NCAP>
__global__ __launch_bounds__(64 * kRefineWaves) void k_refine(uavhip_env env, int stride, int S, int max_sweeps,
                                                              const int* ain, int* aout, double* __restrict__ J,
                                                              int* __restrict__ covered, int* __restrict__ stats) {
    static_assert(NCAP == 0 || TPL == 1, "the register column is the one-target-per-lane path");
    const int s = blockIdx.x * kRefineWaves + (threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    if (s >= S) return;
    const int N = env.N, M = env.M;
    const long long e = (long long)s * stride;
    const long long sb =
        (env.scene_buffers == 2 ? (long long)(env.istate[e * UAVHIP_IST_COUNT + UAVHIP_IST_SCENE_SEL] & 1) * env.E : 0) + e;
    const double omega = env.prm[UAVHIP_PRM_OMEGA];
    const double* __restrict__ pd = env.p_dmg + sb * N * M;

    double v[TPL];
    int id[TPL];
#pragma unroll
    for (int j = 0; j < TPL; ++j) {
        const int t = lane + kWave * j;
        v[j] = t < M ? env.tgt_value[sb * M + t] : 0.0;
        id[j] = t < M ? env.tgt_id[sb * M + t] : 0;
    }
    const bool isu = lane < N;
    const double pen = isu ? env.p_pen[sb * N + lane] : 0.0;
    const double cost = isu ? env.uav_cost[sb * N + lane] : 0.0;
    const double wc = omega * cost;

    // target ids -> list indices: a ballot against the lanes' ids, the lowest list index first
    int a = -1, invalid = 0;
    if (ain) {
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

    double om[NCAP > 0 ? NCAP : 1];
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

    // Q[j] = product of (1 - P[w][t]) over w != skip with a[w] == t, ascending w, from 1.0;
    // cnt[j] = the number of those w
    auto build_q = [&](int skip, double(&Q)[TPL], int(&cnt)[TPL]) {
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
    };

    int sweeps = 0, moves = 0, converged = 1;
    while (sweeps < max_sweeps) {
        int moved = 0;
        for (int u = 0; u < N; ++u) {
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
                    if (g[j] > bg) {
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
    if (stats && lane < 4)
        stats[(long long)s * 4 + lane] = lane == 0 ? sweeps : lane == 1 ? moves : lane == 2 ? converged : invalid;
}

}  // namespace
}  // namespace uavhip

extern "C" int uavhip_refine_assignments(const uavhip_env* env, int32_t env_stride, int32_t S, int32_t max_sweeps,
                                         const int32_t* assignment_in, int32_t* assignment_out, double* J,
                                         int32_t* covered, int32_t* stats, uavhip_stream_t stream) {
    using namespace uavhip;
    if (const int rc = validate_env(env, false)) {
        char why[256];
        snprintf(why, sizeof why, "%s", uavhip_last_error());
        set_error("uavhip_refine_assignments: %s", why);
        return rc;
    }
    if (env_stride < 1 || S < 1 || (long long)(S - 1) * env_stride >= env->E || max_sweeps < 0 || !assignment_out ||
        !J || !covered) {
        set_error("uavhip_refine_assignments: need env_stride=%d >= 1, S=%d >= 1, (S - 1) * env_stride < E=%d, "
                  "max_sweeps=%d >= 0 and assignment_out/J/covered non-NULL",
                  env_stride, S, env->E, max_sweeps);
        return UAVHIP_EINVAL;
    }
    const dim3 grid((S + kRefineWaves - 1) / kRefineWaves), block(64 * kRefineWaves);
    const hipStream_t st = (hipStream_t)stream;
#define UAVHIP_REFINE(TPL, NCAP)                                                                                \
    hipLaunchKernelGGL((k_refine<TPL, NCAP>), grid, block, 0, st, *env, (int)env_stride, (int)S, (int)max_sweeps, \
                       assignment_in, assignment_out, J, covered, stats)
    if (env->M > kWave)
        UAVHIP_REFINE(2, 0);
    else if (env->N <= 8)
        UAVHIP_REFINE(1, 8);
    else if (env->N <= 16)
        UAVHIP_REFINE(1, 16);
    else if (env->N <= 32)
        UAVHIP_REFINE(1, 32);
    else
        UAVHIP_REFINE(1, 0);
#undef UAVHIP_REFINE
    return check_launch("k_refine");
}
