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
//
// Below the scan, what k_search_constrained and k_search_multistart (search_multistart.hip) share: the
// start of the constrained rule (start_limits) and the eight counters a constrained row reports
// (search_stat). The loop of phases, scans and exchanges they also share is search_loop_body.hpp.
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

// RowLimits from the row's arrays (a NULL array constrains nothing), then the start of the rule on
// r.a: pass 1 counts the fixed UAVs on their targets and their conflicts, pass 2 visits the free
// ones in ascending u and drops a pair that is not allowed or whose target is full so far.
template <int TPL, int NR>
__device__ __forceinline__ void start_limits(RefineRow<TPL, NR, true>& r, int s, const uint8_t* __restrict__ allowed,
                                             const uint8_t* __restrict__ fixed, const int* __restrict__ capacity,
                                             int& dropped, int& conflicts) {
    const int N = r.N, M = r.M, lane = r.lane;
    int cnt[TPL];
#pragma unroll
    for (int j = 0; j < TPL; ++j) {
        const int t = lane + kWave * j;
        unsigned long long ok = ~0ull;
        if (allowed) {
            ok = 0;
            const uint8_t* row = allowed + (long long)s * N * M;
            for (int u = 0; u < N; ++u)
                if (t < M && row[u * M + t]) ok |= 1ull << u;
        }
        r.lim.ok[j] = ok;
        int cap = 0x7fffffff;
        if (capacity && t < M) cap = capacity[(long long)s * M + t];
        r.lim.cap[j] = cap < 0 ? 0 : cap;
        cnt[j] = 0;
    }
    r.lim.fixed = ballot(fixed && r.isu && fixed[(long long)s * N + lane]);

    dropped = 0;
    conflicts = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int u = 0; u < N; ++u) {
            if ((int)(r.lim.fixed >> u & 1) == pass) continue;  // pass 0: the fixed UAVs; pass 1: the free ones
            const int au = readlane_i(r.a, u);
            if (au < 0) continue;
            unsigned long long pair = 0, room = 0;  // nonzero: u may take au; au has room so far
#pragma unroll
            for (int j = 0; j < TPL; ++j) {
                const bool mine = lane + kWave * j == au;
                pair |= ballot(mine && (r.lim.ok[j] >> u & 1));
                room |= ballot(mine && cnt[j] < r.lim.cap[j]);
            }
            if (pass == 0) {
                conflicts += (pair == 0) + (room == 0);
            } else if (pair == 0 || room == 0) {
                if (lane == u) r.a = -1;
                ++dropped;
                continue;
            }
#pragma unroll
            for (int j = 0; j < TPL; ++j)
                if (lane + kWave * j == au) ++cnt[j];
        }
    }
}

// column `lane` < 8 of a constrained row's stats
template <int TPL, int NR, bool LIM>
__device__ __forceinline__ int search_stat(const RefineRow<TPL, NR, LIM>& r, int lane, int exchanges, int scan_clean,
                                           int dropped, int conflicts) {
    return lane == 0   ? r.sweeps
           : lane == 1 ? r.moves
           : lane == 2 ? r.converged
           : lane == 3 ? r.invalid
           : lane == 4 ? exchanges
           : lane == 5 ? scan_clean
           : lane == 6 ? dropped
                       : conflicts;
}

}  // namespace uavhip
