// exact_device.hpp -- one tile of one stage of the subset DP, shared by k_exact_stage (exact.hip,
// uavhip_solve_exact: the bits are all N UAVs) and k_exact_free_stage (exact_free.hip,
// uavhip_solve_exact_free: the bits are a row's free UAVs). Both translation units are built with
// -ffp-contract=off; the rule is in include/uavhip.h and the tile's plan at the top of exact.hip.
// What a caller gives the tile is what differs between the two: the number of bits, the value of the
// target (v[t], or v[t] q_fix[t] with held UAVs on it) and, in lane b, 1 - P[.][t] and omega c[.] of
// the UAV of bit b.
#pragma once
#include "refine_device.hpp"

namespace uavhip {
namespace {

constexpr int kExactLowBits = 10;
constexpr int kExactTile = 1 << kExactLowBits;

struct ExactMask {
    uint16_t may, must;  // bit b: the UAV of bit b may be on the target (free and allowed, or fixed to it) / is fixed to it
    int32_t cap;         // the most bits of a set on the target
};

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

// ------------------------------------------------------------------ one tile of one stage
// The 64-thread workgroup's tile: the 2^L states of high part Sh of tables over nb bits, L = min(nb, 10).
// v: the target's value; om, wc: lane b < nb holds 1 - P[.][t] and omega c[.] of the UAV of bit b (1.0
// and 0.0 in the other lanes); mk: the target's sets; dprev / dnext: D_t / D_{t+1} [2^nb]; choice: the
// stage's choice_t [2^nb]; first: D_t is all zero and is not read.
__device__ __forceinline__ void exact_stage_tile(int nb, unsigned Sh, int first, double v, double om, double wc,
                                                 const ExactMask mk, const double* dprev, double* dnext,
                                                 uint16_t* choice) {
    __shared__ double tile[kExactTile], comb[kExactTile], accv[kExactTile];
    __shared__ uint16_t accc[kExactTile];
    const int lane = threadIdx.x;
    const int L = nb < kExactLowBits ? nb : kExactLowBits, H = nb - L, nl = 1 << L;
    const double ninf = -__builtin_huge_val();

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

// ------------------------------------------------------------------ host: what the two entry points share
// The caller's workspace: non-NULL, 16-byte aligned, at least one row of row_bytes. `sizer` names the
// function that sizes it and `row` (a format and its values) the row, for the message.
inline int check_dp_workspace(const char* fn, const void* workspace, int64_t workspace_bytes, long long row_bytes,
                              const char* sizer, const char* row, ...) {
    if (workspace && !((uintptr_t)workspace & 15) && workspace_bytes >= row_bytes) return UAVHIP_OK;
    char c[64];
    va_list ap;
    va_start(ap, row);
    vsnprintf(c, sizeof c, row, ap);
    va_end(ap);
    set_error("%s: workspace=%p (16-byte aligned) of %lld bytes holds no row: one row of %s needs %lld (%s)", fn,
              workspace, (long long)workspace_bytes, c, row_bytes, sizer);
    return UAVHIP_EINVAL;
}

// body(s0, R) on the S rows in chunks of the `fit` >= 1 rows the workspace holds; the first failure ends it
template <class Body>
inline int for_row_chunks(int S, long long fit, Body body) {
    const int chunk = (int)(fit < S ? fit : S);
    for (int s0 = 0; s0 < S; s0 += chunk)
        if (const int rc = body(s0, S - s0 < chunk ? S - s0 : chunk)) return rc;
    return UAVHIP_OK;
}

}  // namespace
}  // namespace uavhip
