// search.hip -- exchange-move local search on J(X) (uavhip_search_assignments): the best-response
// sweeps of uavhip_refine_assignments, and, where no single move improves J any more, the best
// pairwise exchange -- UAVs i and j swap their targets, one of which may be "none" -- after which the
// sweeps run again; until neither neighbourhood improves J or max_exchanges exchanges are made. The
// rule is in include/uavhip.h. Built with -ffp-contract=off: the tests compare assignments bit for
// bit with a Python restatement of the rule.
//
// One wave per row, four per workgroup; the row's registers and the sweeps are RefineRow
// (refine_device.hpp), k_refine's own. The scan over the pairs, per lane u < N once per scan:
//   Po[u] = P[u][a[u]]                                                     (one gathered load)
//   Qo[u] = product of (1.0 - Po[k]) over k != u with a[k] == a[u], ascending k
//           (N readlanes of a[k] and 1.0 - Po[k], a predicated multiply each)
//   vt[u] = v[a[u]]                                                        (a shuffle)
//   gown[u] = g(u, a[u], Qo[u])
// then a uniform loop over i: lane j > i evaluates d(i, j) from the uniform a[i], Qo[i], gown[i],
// v[a[i]], p_pen[i], w c[i], its own a[j], Qo[j], gown[j], vt[j], p_pen[j], w c[j] and two gathered
// loads, p_dmg[j][a[i]] and p_dmg[i][a[j]] -- about N gathered loads per UAV and scan. The lane keeps
// its best over i (strict >: the lowest i), a six-step butterfly on (d, i, j) the lowest (i, j)
// among equal d. No LDS, no atomics, nothing shared between waves; the env and the scene are only read.
#include "refine_device.hpp"

namespace uavhip {
namespace {

// value of target t >= 0 from the lanes that own it, t per lane
template <int TPL>
__device__ __forceinline__ double value_of(const double (&v)[TPL], int t) {
    double x = __shfl(v[0], t & (kWave - 1));
    if constexpr (TPL == 2) {
        const double hi = __shfl(v[1], t & (kWave - 1));
        x = t >= kWave ? hi : x;
    }
    return x;
}

template <int TPL, int NR>
__global__ __launch_bounds__(64 * kRefineWaves) void k_search(uavhip_env env, int stride, int S, int max_exchanges,
                                                              int max_sweeps, const int* ain, int* aout,
                                                              double* __restrict__ J, int* __restrict__ covered,
                                                              int* __restrict__ stats) {
    const int s = blockIdx.x * kRefineWaves + (threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    if (s >= S) return;
    RefineRow<TPL, NR> r;
    r.load(env, s, stride, lane);
    r.convert(ain, s);
    r.load_columns();
    const int N = r.N, M = r.M;

    int exchanges = 0, scan_clean = 0;
    for (;;) {
        r.phase(max_sweeps);
        if (max_exchanges == 0) break;

        // per-UAV terms of this scan
        const int t = r.isu ? r.a : -1;
        const int tc = t < 0 ? 0 : t;  // a valid index for the loads and shuffles of an idle lane
        const double Po = t >= 0 ? r.pd[lane * M + tc] * r.pen : 0.0;
        const double omo = 1.0 - Po;
        double Qo = 1.0;
        for (int k = 0; k < N; ++k) {
            const int ak = readlane_i(t, k);
            if (ak < 0) continue;
            const double ok = readlane_d(omo, k);
            if (ak == t && k != lane) Qo = Qo * ok;
        }
        const double vt = value_of<TPL>(r.v, tc);
        const double vq = vt * Qo;
        const double gown = t >= 0 ? vq * Po - r.wc : 0.0;

        double bd = -__builtin_huge_val();
        int bi = 0x7fffffff;
        for (int i = 0; i + 1 < N; ++i) {
            const int si = readlane_i(t, i);
            const int sc = si < 0 ? 0 : si;
            const double Qi = readlane_d(Qo, i), gi = readlane_d(gown, i);
            const double peni = readlane_d(r.pen, i), wci = readlane_d(r.wc, i);
            double vs;
            if constexpr (TPL == 2)
                vs = readlane_d(sc >= kWave ? r.v[1] : r.v[0], sc & (kWave - 1));
            else
                vs = readlane_d(r.v[0], sc);
            if (lane > i && lane < N && t != si) {
                // j = lane takes s = a[i], i takes t = a[j]
                const double gjs = si >= 0 ? (vs * Qi) * (r.pd[lane * M + sc] * r.pen) - r.wc : 0.0;
                const double git = t >= 0 ? vq * (r.pd[i * M + tc] * peni) - wci : 0.0;
                const double d = (gjs + git) - (gi + gown);
                if (d > bd) {
                    bd = d;
                    bi = i;
                }
            }
        }
        int bj = lane;
#pragma unroll
        for (int m = 1; m < kWave; m <<= 1) {
            const double d_o = __shfl_xor(bd, m);
            const int i_o = __shfl_xor(bi, m), j_o = __shfl_xor(bj, m);
            if (d_o > bd || (d_o == bd && (i_o < bi || (i_o == bi && j_o < bj)))) {
                bd = d_o;
                bi = i_o;
                bj = j_o;
            }
        }
        bd = readlane_d(bd, 0);
        bi = readlane_i(bi, 0);
        bj = readlane_i(bj, 0);
        if (!(bd > 0.0)) {
            scan_clean = 1;
            break;
        }
        if (exchanges == max_exchanges) break;
        const int ai = readlane_i(r.a, bi), aj = readlane_i(r.a, bj);
        if (lane == bi) r.a = aj;
        if (lane == bj) r.a = ai;
        ++exchanges;
    }

    r.finish(s, aout, J, covered);
    if (stats && lane < 6)
        stats[(long long)s * 6 + lane] = lane == 0   ? r.sweeps
                                         : lane == 1 ? r.moves
                                         : lane == 2 ? r.converged
                                         : lane == 3 ? r.invalid
                                         : lane == 4 ? exchanges
                                                     : scan_clean;
}

}  // namespace
}  // namespace uavhip

extern "C" int uavhip_search_assignments(const uavhip_env* env, int32_t env_stride, int32_t S, int32_t max_exchanges,
                                         int32_t max_sweeps, const int32_t* assignment_in, int32_t* assignment_out,
                                         double* J, int32_t* covered, int32_t* stats, uavhip_stream_t stream) {
    using namespace uavhip;
    if (const int rc = check_rows("uavhip_search_assignments", env, env_stride, S,
                                  max_exchanges >= 0 && max_sweeps >= 0 && assignment_out && J && covered,
                                  "max_exchanges=%d >= 0, max_sweeps=%d >= 0", max_exchanges, max_sweeps))
        return rc;
    UAVHIP_ROWS_LAUNCH(env, S, (k_search<TPL, NCAP>), stream, *env, (int)env_stride, (int)S, (int)max_exchanges,
                       (int)max_sweeps, assignment_in, assignment_out, J, covered, stats);
    return check_launch("k_search");
}
