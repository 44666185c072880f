// search_device.hpp -- the scan of the exchange-move search, shared by k_search (search.hip) and
// k_search_constrained (search_constrained.hip): the best pairwise exchange of one row, on RefineRow
// (refine_device.hpp). The rule is in include/uavhip.h.
//
// The scan, per lane u < N once per scan:
//   Po[u] = P[u][a[u]]                                                     (one gathered load)
//   Qo[u] = product of (1.0 - Po[k]) over k != u with a[k] == a[u], ascending k
//           (N readlanes of a[k] and 1.0 - Po[k], a predicated multiply each)
//   vt[u] = v[a[u]]                                                        (a shuffle)
//   gown[u] = g(u, a[u], Qo[u])
// then a uniform loop over i: lane j > i evaluates d(i, j) from the uniform a[i], Qo[i], gown[i],
// v[a[i]], p_pen[i], w c[i], its own a[j], Qo[j], gown[j], vt[j], p_pen[j], w c[j] and two gathered
// loads, p_dmg[j][a[i]] and p_dmg[i][a[j]] -- about N gathered loads per UAV and scan. The lane keeps
// its best over i (strict >: the lowest i), a six-step butterfly on (d, i, j) the lowest (i, j)
// among equal d.
// With LIM (RowLimits) a pair needs both UAVs free, j allowed on a[i] -- bit j of the mask lane a[i]
// holds, a uniform readlane per i -- and i allowed on a[j] -- bit i of the mask of a[j], which lane j
// fetches once per scan by a shuffle. A swap keeps every target's count: capacity is not looked at.
#pragma once
#include "refine_device.hpp"

namespace uavhip {

// what the lanes that own target t >= 0 hold for it, t per lane
template <int TPL, class T>
__device__ __forceinline__ T value_of(const T (&v)[TPL], int t) {
    T x = __shfl(v[0], t & (kWave - 1));
    if constexpr (TPL == 2) {
        const T hi = __shfl(v[1], t & (kWave - 1));
        x = t >= kWave ? hi : x;
    }
    return x;
}

__device__ __forceinline__ unsigned long long readlane_ull(unsigned long long v, int l) {
    return ((unsigned long long)readlane_u((uint32_t)(v >> 32), l) << 32) | readlane_u((uint32_t)v, l);
}

// the pair (bi, bj) with the largest d, and d; bd = -inf without a pair. Every lane gets the result.
template <int TPL, int NR, bool LIM>
__device__ __forceinline__ void best_exchange(const RefineRow<TPL, NR, LIM>& r, double& bd, int& bi, int& bj) {
    const int N = r.N, M = r.M, lane = r.lane;
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
    unsigned long long okt = ~0ull;  // the UAVs that may take t
    bool free_j = true;
    if constexpr (LIM) {
        const unsigned long long m = value_of<TPL>(r.lim.ok, tc);
        okt = t >= 0 ? m : ~0ull;
        free_j = !(r.lim.fixed >> lane & 1);
    }

    bd = -__builtin_huge_val();
    bi = 0x7fffffff;
    for (int i = 0; i + 1 < N; ++i) {
        if constexpr (LIM) {
            if (r.lim.fixed >> i & 1) continue;
        }
        const int si = readlane_i(t, i);
        const int sc = si < 0 ? 0 : si;
        const double Qi = readlane_d(Qo, i), gi = readlane_d(gown, i);
        const double peni = readlane_d(r.pen, i), wci = readlane_d(r.wc, i);
        double vs;
        if constexpr (TPL == 2)
            vs = readlane_d(sc >= kWave ? r.v[1] : r.v[0], sc & (kWave - 1));
        else
            vs = readlane_d(r.v[0], sc);
        bool may = true;
        if constexpr (LIM) {
            unsigned long long oks;  // the UAVs that may take s = a[i]
            if constexpr (TPL == 2)
                oks = readlane_ull(sc >= kWave ? r.lim.ok[1] : r.lim.ok[0], sc & (kWave - 1));
            else
                oks = readlane_ull(r.lim.ok[0], sc);
            may = free_j && (si < 0 || (oks >> lane & 1)) && (okt >> i & 1);
        }
        if (may && lane > i && lane < N && t != si) {
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
    bj = lane;
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
}

}  // namespace uavhip
