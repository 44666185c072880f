// policy.hip -- K4: fused TransformerActorCritic forward (networks/transformer_net.py:15-144) on
// gfx950, fp32-accurate (the reference's dtype): every encoder GEMM as split products on the f16
// MFMA (v_mfma_f32_16x16x32_f16, each operand as two fp16 planes x1 = f16(x), x2 = f16((x - x1) 2^11),
// three MFMAs per block, fp32 accumulation), the embeddings (K = 14) and the heads on
// the f32 MFMA (v_mfma_f32_16x16x4_f32, exact fp32 products). Range of the split operands: 2^-22
// relative per product for |x| in [2^-14, 65504]; below 2^-14 an absolute floor of ~2^-36 (the
// backward therefore carries its gradients pre-scaled, BwdIO::gscale); from 65520 up the planes are
// inf / -inf and every output that reads them is non-finite (common.hpp f16_lo; the ReLUs keep NaN,
// relu_nan), never a finite wrong value.
//
// Work decomposition (MI355X-first):
//  * one workgroup = 4 waves = 16 samples = 80 tokens, token index tok = s * 16 + p (s = window
//    position, p = sample): every 16-column MFMA tile is one window position of the 16 samples,
//    so the last position (the only one the heads read, transformer_net.py:106,114) is exactly
//    column tile 4. B = 4096 -> 256 workgroups = one per CU.
//  * GEMMs are computed transposed, Y^T = W . X^T: the weight rows (Linear's [out][in] layout,
//    contiguous in k) are the A operand, streamed from L2 as float4 (4 k per lane = 4 MFMAs);
//    activations live in LDS as [tok][feature] rows and are the B operand, read as float4; the
//    accumulator (feature rows x token columns) is stored back as one float4 per lane.
//    Both operands use the same k permutation (k = 16*i + 4*(lane>>4) + j for MFMA j), so the
//    sum is over every k exactly once.
//  * the four waves split the output features of every GEMM; attention (5 x 5 per sample and
//    head, far too small for MFMA), LayerNorm and the 128->64->{2,1} heads run on the VALU.
//  * last-layer pruning: in the final encoder layer of each trunk only K and V are formed for
//    all 80 tokens; Q, attention, out-projection, LayerNorms and the FFN run for column tile 4
//    only (2.45 instead of 4.04 MFLOP per sample; numerically identical outputs).
//  * sampling: a = (u < p0) ? 0 : 1 with u ~ Philox(seed, offset + b) (not torch's RNG stream;
//    parity is defined on logits / logp / value / entropy for given actions).
//
// The forward's device code, which rollout_steps.hip compiles too, lives in headers by role:
// policy_core.hpp (primitives), policy_encoder.hpp (an encoder trunk), policy_block.hpp (the workgroup's
// forward and k_policy_forward), policy_steps.hpp (the interface to rollout_steps.hip's multi-step
// kernels). This file holds what only this translation unit builds: the loss-partials and ring-fill
// kernels, the training backward (K6), the position-split training kernels (K7), the weight pack /
// split / range kernels, the launchers and the C ABI.
#include <cstdarg>
#include <cstdio>

#include "policy_steps.hpp"  // policy_core.hpp, policy_encoder.hpp, policy_block.hpp, the multi-step launchers

namespace uavhip {
namespace pol {

// Trunk split: the same partials once both trunks' workgroups have written smp[5..7].
__global__ __launch_bounds__(64) void k_loss_partials(const TrainIO io) {
    __shared__ float red[5 * SPW];
    const int b0 = blockIdx.x * SPW;
    if (TIDX() < SPW) {
        const float* o = io.smp + (size_t)(b0 + TIDX()) * 8;
        const float eps_clip = hyper_f32(io.hyper, UAVHIP_HP_EPS_CLIP, io.eps_clip);
        const float oi[5] = {o[0], o[1], o[2], o[3], o[4]};
        loss_terms(oi, o[5], o[6], o[7], eps_clip, red + 4 * TIDX(), red + 4 * SPW + TIDX());
    }
    __syncthreads();
    loss_block_sums(TID_C red, io.fpart, io.vpart, blockIdx.x);
}

// Ring fill of one trunk: u rows of positions 0-3 of the workgroup's 16 windows -> slots
// (g + 1 + s) mod 5, the same GEMM (k order, bias add) as the forward's new-row u. Every global
// operand of a trunk's fill -- the embedding's, the wave's in_proj row tiles (all k blocks) and
// their biases -- is one FillPre, loaded ahead (k_policy_rows_fill: the actor's before the window
// rows, the critic's before the actor's GEMMs), so a trunk's fill waits for one L2 round trip
// instead of one per row tile and k-block pair.
template <int trunk>
struct FillPre {
    static constexpr int NP = row_parts<trunk>();
    using W = std::conditional_t<split_ring<trunk>(), HPre<4>, APre<KB>>;
    EmbPre ep;
    W w[NP];
    f32x4 bb[NP];
};
template <int trunk>
__device__ __forceinline__ void fill_load_w(FillPre<trunk>& r, const float* __restrict__ P) {
    constexpr int NP = row_parts<trunk>(), P0 = 3 - NP;
    const int g = lane_id() >> 4, wv = tid_x() >> 6;
    const float* bin = P + kOffs.o[layer_param(trunk, 0, INB)];
#pragma unroll
    for (int j = P0; j < 3; ++j) {
        const int row = j * D + 16 * wv;
        if constexpr (split_ring<trunk>()) r.w[j - P0] = hprefetch<4>(P, split_slot(layer_param(trunk, 0, INW)), D, row, 0);
        else r.w[j - P0] = prefetch<KB>(P + kOffs.o[layer_param(trunk, 0, INW)], D, row, 0);
        r.bb[j - P0] = *reinterpret_cast<const f32x4*>(bin + row + 4 * g);
    }
}
// `after_first` runs after the first row tile's GEMM (the next trunk's weights are issued there,
// once this trunk's first tile has released its registers).
template <int trunk, class F>
__device__ void rows_fill_trunk(Smem& sm, const float* __restrict__ P, const FillPre<trunk>& pre, const RowIO& rio,
                                int b0, F after_first) {
    constexpr int NP = row_parts<trunk>(), P0 = 3 - NP, ROFF = trunk == kActorTrunk ? 0 : 2 * D;
    const float* Win = P + kOffs.o[layer_param(trunk, 0, INW)];
    const int l = lane_id(), i16 = l & 15, g = l >> 4, wv = tid_x() >> 6;
    embed_apply<trunk, false, kEmbRows>(sm, pre.ep);
    __syncthreads();
    float* slots = rio.rp + kPposFloats;
#pragma unroll
    for (int j = P0; j < 3; ++j) {
        const int row = j * D + 16 * wv;
        f32x4 acc[S - 1];
        zero(acc);
        if constexpr (split_ring<trunk>()) {  // the forward's new-row GEMM as split products: the same sums
            constexpr int si = split_slot(layer_param(trunk, 0, INW));
            f32x4 lo[S - 1];
            zero(lo);
            hgemm_tile<S - 1, 4>(acc, lo, pre.w[j - P0], P, si, D, row, 0, reinterpret_cast<const _Float16*>(sm.ctx), 0);
#pragma unroll
            for (int s = 0; s < S - 1; ++s) acc[s] = (acc[s] + lo[s] * kLoScale) * es_factor<trunk, 1>(sm, s * SPW + i16);
        } else {
            gemm_tile<S - 1, KB>(acc, pre.w[j - P0], Win, D, row, 0, sm.ctx, LDH, 0);
        }
        if (j == P0) after_first();
        const f32x4 bb = pre.bb[j - P0];
        const int b = b0 + i16;
        if (b < rio.B) {
#pragma unroll
            for (int s = 0; s < S - 1; ++s)
                *reinterpret_cast<f32x4*>(slots + ((size_t)((rio.g + 1 + s) % 5) * rio.B + b) * kRowFloats + ROFF +
                                          (j - P0) * D + 16 * wv + 4 * g) = acc[s] + bb;
        }
    }
    __syncthreads();  // sm.ctx is the next trunk's embedding
}

// Win pos_s of one trunk -> rp[trunk][s][384] (no bias): pos rows as activation tile columns 0-4;
// part j = rows [128 j, 128 j + 128) (Q, K or V), its weight blocks loaded before the pos rows.
constexpr int kPposParts = 6;  // (trunk, j) pairs
template <int trunk>
__device__ void rows_ppos_part(Smem& sm, const float* __restrict__ P, float* out, int j) {
    const float* Win = P + kOffs.o[layer_param(trunk, 0, INW)];
    const float* pos = P + kOffs.o[trunk + POS];
    const int l = lane_id(), i16 = l & 15, g = l >> 4, wv = tid_x() >> 6;
    const int row = j * D + 16 * wv;
    const APre<KB> pw = prefetch<KB>(Win, D, row, 0);
    for (int i = tid_x(); i < SPW * D; i += NTHR) {
        const int t = i / D, k = i - t * D;
        sm.h[t * LDH + k] = t < S ? pos[t * D + k] : 0.f;
    }
    __syncthreads();
    f32x4 acc[1];
    zero(acc);
    gemm_tile<1, KB>(acc, pw, Win, D, row, 0, sm.h, LDH, 0);
    if (i16 < S) *reinterpret_cast<f32x4*>(out + i16 * 3 * D + row + 4 * g) = acc[0];
}

// uavhip_policy_forward_rows with fill: rebuilds the ring rows of positions 0-3 of every window
// (blocks < nb) and the Win pos_s table (blocks < kPposParts, one (trunk, part) each, after their
// fill: the grid is max(nb, kPposParts) blocks). The table used to be one extra block of its own:
// with one workgroup per CU it waited for a free CU and then ran six serial GEMMs, 28 us per
// launch against ~10 us now (r04x / r04y).
__global__ __launch_bounds__(NTHR) void k_policy_rows_fill(const float* __restrict__ P,
                                                           const float* __restrict__ states, const RowIO rio) {
    __shared__ __attribute__((aligned(16))) Smem sm;
    const int nb = (rio.B + SPW - 1) / SPW;
    load_rtab(sm, P);
    if ((int)blockIdx.x < nb) {
        const int b0 = blockIdx.x * SPW;
        FillPre<kActorTrunk> fa;
        FillPre<kCriticTrunk> fc;
        fa.ep = embed_load<kActorTrunk>(P);
        fill_load_w(fa, P);
        fc.ep = embed_load<kCriticTrunk>(P);
        for (int i = tid_x(); i < (S - 1) * SPW * LDX; i += NTHR) {  // positions 0-3 only
            const int t = i / LDX, k = i - t * LDX, s = t / SPW, p = t - s * SPW;
            const float x = (k < IN && b0 + p < rio.B) ? states[((size_t)(b0 + p) * S + s) * IN + k] : 0.f;
            sm.x[i] = x;
            const float rmax = row16_max(fabsf(x));  // the row's range (one 16-lane row per token)
            if (k == 0) {
                sm.tmax[t] = rmax;
#pragma unroll
                for (int ti = 0; ti < 2; ++ti)  // as gather_windows
                    sm.es[ti][t] = (signed char)range_exp(
                        e_bound_v(range_entry(P + kRangeOff, kRgE + 2 * ti), range_entry(P + kRangeOff, kRgE + 2 * ti + 1),
                                  rmax));
            }
        }
        __syncthreads();
        rows_fill_trunk<kActorTrunk>(sm, P, fa, rio, b0, [&] { fill_load_w(fc, P); });
        rows_fill_trunk<kCriticTrunk>(sm, P, fc, rio, b0, [] {});  // ends with a barrier
    }
    if ((int)blockIdx.x < kPposParts) {  // block-uniform
        const int t = blockIdx.x;
        if (t < 3) rows_ppos_part<kActorTrunk>(sm, P, rio.rp, t);
        else rows_ppos_part<kCriticTrunk>(sm, P, rio.rp + S * 3 * D, t - 3);
    }
}

// ================================================================== K6: fused training backward
// Mirror of the forward for one 16-sample workgroup: gradients flow through the LDS-resident
// [tok][feature] rows, the dX GEMMs run transposed on the MFMA with the transposed weights
// (policy_pack_transposed) as A operands, and only the dY operands of the weight-gradient GEMMs
// (df, du, dz1, dqkv) plus per-workgroup LayerNorm / embedding partials go to HBM.
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ float add_ror4(float v) {  // row_ror:4 inside each row of 16 lanes
    return v + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x124, 0xF, 0xF, true));
}
__device__ __forceinline__ float add_ror8(float v) {
    return v + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x128, 0xF, 0xF, true));
}
__device__ __forceinline__ float row16_sum(float v) { return add_ror8(add_ror4(add_xor2(add_xor1(v)))); }
__device__ __forceinline__ float hsum(f32x4 v) { return (v.x + v.y) + (v.z + v.w); }

// LayerNorm backward (torch's formula) on LDS rows, tokens [t0, TOK), 16 lanes per token and 8
// features per lane: g = src * w; dz = rstd * (g - mean(g) - xhat * mean(g * xhat)) -> dst (LDS)
// and gout (workspace rows). Workgroup partials, reduced over the 32 lane groups through `scratch`
// (12 KiB floats): dw = sum src * xhat, db = sum src -> part[0..127], [128..255]; the bias
// gradient of the linear that produced the LayerNorm input, sum dz -> bias[0..127]. Ends without a
// barrier after the partials are written (scratch is read until then).
// Its global operands -- the weight and this lane group's (<= 3) tokens' xhat rows and 1/std -- in
// one round trip, issued by the caller ahead of time (ln_bwd_load) so the HBM latency hides under
// the preceding phase.
constexpr int kLnIt = (TOK + NTHR / 16 - 1) / (NTHR / 16);
struct LnBwdPre {
    f32x4 w0, w1, X0[kLnIt], X1[kLnIt];
    float RS[kLnIt];
};
__device__ __forceinline__ void ln_bwd_load(LnBwdPre& a, const float* __restrict__ xhat, const float* __restrict__ rstd,
                                            const float* __restrict__ w, int t0, int b0, bool compact, int t1 = TOK) {
    const int f0 = 8 * (tid_x() & 15), grp = tid_x() >> 4;
    a.w0 = ld4(w + f0);
    a.w1 = ld4(w + f0 + 4);
#pragma unroll
    for (int it = 0; it < kLnIt; ++it) {
        const int tok = t0 + grp + it * (NTHR / 16);
        if (tok < t1) {  // wave-uniform
            const size_t r = (size_t)orow(tok, b0, compact);
            a.X0[it] = ld4(xhat + r * D + f0);
            a.X1[it] = ld4(xhat + r * D + f0 + 4);
            a.RS[it] = rstd[r];
        }
    }
}
// dst receives the two fp16 planes of the split products (the next GEMM's operand).
__device__ void ln_bwd_lds(const float* src, float* dst, const LnBwdPre& a, float* __restrict__ gout,
                           float* __restrict__ part, float* __restrict__ bias, int t0, int b0, bool compact,
                           float* scratch, int t1 = TOK) {
    const int j = tid_x() & 15, grp = tid_x() >> 4;
    const int f0 = 8 * j;
    const f32x4 w0 = a.w0, w1 = a.w1;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 pw0 = zero4, pw1 = zero4, pb0 = zero4, pb1 = zero4, pd0 = zero4, pd1 = zero4;
    constexpr int kIt = kLnIt;
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
        const int tok = t0 + grp + it * (NTHR / 16);
        if (tok >= t1) continue;
        const size_t r = (size_t)orow(tok, b0, compact);
        const f32x4 g0 = ld4(src + tok * LDH + f0), g1 = ld4(src + tok * LDH + f0 + 4);
        const f32x4 x0 = a.X0[it], x1 = a.X1[it];
        const float rs = a.RS[it];
        const f32x4 gw0 = g0 * w0, gw1 = g1 * w1;
        const float m1 = row16_sum(hsum(gw0) + hsum(gw1)) * (1.0f / D);
        const float m2 = row16_sum(hsum(gw0 * x0) + hsum(gw1 * x1)) * (1.0f / D);
        const f32x4 d0 = rs * (gw0 - m1 - x0 * m2), d1 = rs * (gw1 - m1 - x1 * m2);
        hsplit_store(reinterpret_cast<_Float16*>(dst), psw(tok, f0), d0);
        hsplit_store(reinterpret_cast<_Float16*>(dst), psw(tok, f0 + 4), d1);
        *reinterpret_cast<f32x4*>(gout + r * D + f0) = d0;
        *reinterpret_cast<f32x4*>(gout + r * D + f0 + 4) = d1;
        pw0 += g0 * x0; pw1 += g1 * x1;
        pb0 += g0; pb1 += g1;
        pd0 += d0; pd1 += d1;
    }
    float* sc = scratch + grp * 3 * D;
    st4(sc + f0, pw0); st4(sc + f0 + 4, pw1);
    st4(sc + D + f0, pb0); st4(sc + D + f0 + 4, pb1);
    st4(sc + 2 * D + f0, pd0); st4(sc + 2 * D + f0 + 4, pd1);
    __syncthreads();
    if (tid_x() < 3 * D) {
        float s4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < NTHR / 16; ++q) s4[q & 3] += scratch[q * 3 * D + tid_x()];
        const float tot = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        if (tid_x() < 2 * D) part[tid_x()] = tot;
        else bias[tid_x() - 2 * D] = tot;
    }
}

// Attention backward for heads [4c, 4c+4), P recomputed from q, k (from the workspace qkv rows);
// with g = d(attention output) of the query rows (sm.ctx):
//   dv_j = sum_i P_ij g_i; dP_ij = g_i . v_j; dS_ij = P_ij (dP_ij - sum_k P_ik dP_ik);
//   dq_i = sum_j dS_ij k_j / 4; dk_j = sum_i dS_ij q_i / 4.
// One (sample, head) task per 8 lanes, 2 of the 16 head dims each (all 512 threads; dot products
// reduced over the 8 lanes with two quad permutes and a half-row mirror). dq | dk | dv -> sm.big
// as fp16 planes and the dqkv rows (attn_out2; dq on the query rows only). Per-wave sums over the
// wave's 2 samples of dq, dk, dv -> scratch [wave][192] (in_proj bias partials).
__device__ __forceinline__ float add_hmirror8(float v) {  // + lane 7 - i within each group of 8
    return v + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, true));
}
__device__ __forceinline__ float sum8(float v) { return add_hmirror8(add_xor2(add_xor1(v))); }
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 ld2(const float* p) { return *reinterpret_cast<const f32x2*>(p); }
// K6 reads the forward's Q | K | V rows (read once, by K6 alone) with non-temporal loads: they do not
// displace the L2 lines the rest of the backward re-reads (same-box, three pairs at minibatch 4096:
// K6 106.7 -> 102.1 us on average, profiles/r06s_train_ab_nt_qkv_loads.txt).
__device__ __forceinline__ f32x2 ld2_once(const float* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(p));
}
__device__ __forceinline__ void st2(float* p, f32x2 v) { *reinterpret_cast<f32x2*>(p) = v; }

// The chunk's saved Q / K / V values of this thread (2 head dims of one (sample, head)), loaded by
// the caller well ahead of attn_bwd_chunk: the rows come from HBM (written by the forward long before).
struct AttnPre {
    f32x2 k[S], v[S], q[S];
};
// qsel >= 0 (position split): the one query position qsel; else every position (full layer) or
// position 4 (pruned layer)
template <bool last>
__device__ __forceinline__ void attn_bwd_load(AttnPre& a, const float* __restrict__ qkv, int c, int b0, int qsel = -1) {
    const int o8 = tid_x() & 7, hh = (tid_x() >> 3) & 3, p = tid_x() >> 5;
    const int col = 64 * c + hh * HD + 2 * o8;
    const size_t rb = (size_t)(b0 + p) * S;
#pragma unroll
    for (int j = 0; j < S; ++j) {
        a.k[j] = ld2_once(qkv + (rb + j) * 3 * D + D + col);
        a.v[j] = ld2_once(qkv + (rb + j) * 3 * D + 2 * D + col);
    }
#pragma unroll
    for (int i = 0; i < S; ++i)
        if (qsel >= 0 ? i == qsel : (!last || i == S - 1)) a.q[i] = ld2_once(qkv + (rb + i) * 3 * D + col);
}
// dq | dk | dv go to sm.big as the two fp16 planes of the W_in^T GEMM's operand -- both planes of a
// token in one row, [tok][plane 1: 192 halves | plane 2: 192 | pad 16] (800-B rows: token i16 at
// bank offset 8 i16, conflict-free ds_read_b128 operand reads) -- and, exact, straight to the dqkv
// rows (position split: dk / dv to kvc instead).
constexpr int kLdbP = 2 * LDB, kPlaneB = 3 * 64;  // halves per row, plane 2 within the row
static_assert(kPlaneB + 3 * 64 <= kLdbP, "both planes in an LDB row");
__device__ __forceinline__ void attn_out2(Smem& sm, float* __restrict__ dqkv, int b0, int tok, int col, int part,
                                          int c, f32x2 v, float* __restrict__ kvc = nullptr, int kblk = 0) {
    _Float16* bp = reinterpret_cast<_Float16*>(sm.big) + tok * kLdbP + part * 64 + col;
    const _Float16 a0 = (_Float16)v.x, a1 = (_Float16)v.y;
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    *reinterpret_cast<f16x2*>(bp) = f16x2{a0, a1};
    *reinterpret_cast<f16x2*>(bp + kPlaneB) = f16x2{f16_lo(v.x, a0), f16_lo(v.y, a1)};
    if (kvc && part > 0)  // position split: this query position's share of every position's dk / dv
        st2(kvc + ((size_t)kblk * TOK + tok) * 2 * D + (part - 1) * D + 64 * c + col, v);
    else
        st2(dqkv + (size_t)trow(tok, b0) * 3 * D + part * D + 64 * c + col, v);
}
template <bool last>
__device__ void attn_bwd_chunk(Smem& sm, const AttnPre& a, int c, float* scratch, int qsel, float* __restrict__ dqkv,
                               int b0, float* __restrict__ kvc, int kblk) {
    const int o8 = tid_x() & 7, hh = (tid_x() >> 3) & 3, p = tid_x() >> 5;
    const int d0 = hh * HD + 2 * o8;
    const int col = 64 * c + d0;
    f32x2 k[S], v[S], dk[S], dv[S];
    bool msk[S];
    f32x2 sdq = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < S; ++j) {
        k[j] = a.k[j];
        v[j] = a.v[j];
        msk[j] = sm.mask[p * S + j] != 0;
        dk[j] = f32x2{0.f, 0.f};
        dv[j] = f32x2{0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < S; ++i) {
        f32x2 dq = {0.f, 0.f};
        if (qsel >= 0 ? i == qsel : (!last || i == S - 1)) {
            // the scores' 1/sqrt(16) on the query (q4 = q / 4: exact), so dk[j] += ds q = (ds 4) q4 and
            // dq = (sum_j (ds 4) k_j) / 4 -- the same values as scaling each score and each ds, without
            // the 2 S multiplies
            const f32x2 q4 = a.q[i] * 0.25f;
            const f32x2 g = ld2(sm.ctx + (i * SPW + p) * LDH + col);
            float pr[S], dp[S];
            float mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                const float part = sum8(q4.x * k[j].x + q4.y * k[j].y);
                pr[j] = msk[j] ? -INFINITY : part;
                mx = j == 0 ? pr[j] : fmaxf(mx, pr[j]);
            }
            float den = 0.f;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                pr[j] = __expf(pr[j] - mx);
                den = j == 0 ? pr[j] : den + pr[j];
            }
            const float inv = att_recip(den);
            float sdp = 0.f;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                pr[j] *= inv;
                dp[j] = sum8(g.x * v[j].x + g.y * v[j].y);
                sdp += pr[j] * dp[j];
            }
#pragma unroll
            for (int j = 0; j < S; ++j) {
                const float ds = pr[j] * (dp[j] - sdp);
                dq += ds * k[j];
                dk[j] += ds * q4;
                dv[j] += pr[j] * g;
            }
            dq *= 0.25f;
            sdq += dq;
        }
        if (qsel >= 0 ? i == qsel : (!last || i == S - 1)) attn_out2(sm, dqkv, b0, i * SPW + p, d0, 0, c, dq);
    }
    f32x2 sk = {0.f, 0.f}, sv = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < S; ++j) {
        attn_out2(sm, dqkv, b0, j * SPW + p, d0, 1, c, dk[j], kvc, kblk);
        attn_out2(sm, dqkv, b0, j * SPW + p, d0, 2, c, dv[j], kvc, kblk);
        sk += dk[j];
        sv += dv[j];
    }
    // the wave's two samples are lanes 32 apart
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        sdq[e] = add_xor32(sdq[e]);
        sk[e] = add_xor32(sk[e]);
        sv[e] = add_xor32(sv[e]);
    }
    if ((tid_x() & 63) < 32) {
        float* row = scratch + (tid_x() >> 6) * 3 * 64;
        st2(row + d0, sdq);
        st2(row + 64 + d0, sk);
        st2(row + 128 + d0, sv);
    }
}

// The embedding backward's global inputs (embed_bwd): this thread's 20 embedding values (the ReLU
// mask) and one float4 of the input windows, loaded by the layer-0 backward right after its last
// GEMM (every weight load of the layer issued: nothing waits behind them), so their latency hides
// under the layer's final residual pass and barrier.
struct EmbBwdPre {
    float ev[TOK / 4];
    f32x4 xv;
};
__device__ __forceinline__ void embed_bwd_load(EmbBwdPre& ep, const float* __restrict__ e, const float* __restrict__ xg,
                                               int b0) {
    const int f = tid_x() & (D - 1), grp = tid_x() >> 7;
#pragma unroll
    for (int i = 0; i < TOK / 4; ++i) ep.ev[i] = e[(size_t)trow(grp + 4 * i, b0) * D + f];
    const int i = tid_x();
    ep.xv = i < TOK * LDX / 4 ? ld4(xg + (size_t)trow(i / (LDX / 4), b0) * 16 + 4 * (i % (LDX / 4)))
                              : f32x4{0.f, 0.f, 0.f, 0.f};
}

enum { kBwdFull = 0, kBwdNoDx = 1, kBwdPos = 2 };  // bwd_layer's MODE
// Backward of one post-LN encoder layer. On entry sm.h holds dL/d(layer output) for the tokens
// >= qtok0; on exit (kBwdFull) sm.h holds dL/d(layer input) for all 80 tokens. Ends with a barrier.
// Every dX GEMM runs as split products on the f16 MFMA -- A = the transposed split copies (PT is
// this layer's packedT, the caller's offset: its split copy at PT + kTSplit), B = planes the
// producing epilogue writes: df (LN2 backward -> sm.ctx), du (-> sm.big / sm.h), dz1 (LN1 backward
// -> sm.h), dq | dk | dv (attention backward -> sm.big, rows of kLdbP halves, attn_out2); the
// residual terms read back from planes are x1 + 2^-11 x2.
// ln2_pre: this layer's LN2-backward operands, already loaded by the caller (nullptr: load here);
// next_load: issues the next phase's global loads behind this layer's last weight loads.
// MODE (the position-split training step, K7 below): kBwdFull = the whole layer; kBwdNoDx = stop after
// the attention backward (dqkv rows and bias partials written; no W_in^T GEMM, no residual -- the
// per-position kernels form dL/d(layer input)); kBwdPos = a full layer for the 16 query tokens of
// ONE window position (tokens [qt, qt + 16), [b * 5 + s] rows, partial row prow): its dq rows go to
// dqkv, its contributions to every position's dk / dv to kvc ([prow][80 tokens][dk 128 | dv 128]).
template <int trunk, int layer, bool last, int TB, class F, int MODE>
__device__ void bwd_layer(Smem& sm, const float* __restrict__ P, const float* __restrict__ PT, const BwdLayerIO& io,
                          int b0, EmbBwdPre* ep, const float* e_emb, const float* xg, const LnBwdPre* ln2_pre,
                          F next_load, int qt, int prow, float* __restrict__ kvc) {
    static_assert(MODE != kBwdPos || !last, "position split: full layers only");
    constexpr int CTQ = (last || MODE == kBwdPos) ? 1 : S;
    const int qtok0 = last ? (S - 1) * SPW : (MODE == kBwdPos ? qt : 0), qtok1 = qtok0 + SPW * CTQ;
    const int qsel = MODE == kBwdPos ? qt / SPW : -1;
    const int sWin = kTSplit + kTWin, sWo = kTSplit + kTWo, sW1 = kTSplit + kTW1, sW2 = kTSplit + kTW2;
    const int wv = tid_x() >> 6, l = lane_id(), i16 = l & 15, g = l >> 4;
    const int fo = 16 * wv + 4 * g;
    const int blk = prow >= 0 ? prow : b0 / SPW;  // this workgroup's partial rows
    float* bias = io.bpart + (size_t)blk * kBiasPart;
    _Float16* const hp = reinterpret_cast<_Float16*>(sm.h);
    _Float16* const bp = reinterpret_cast<_Float16*>(sm.big);
    _Float16* const cp = reinterpret_cast<_Float16*>(sm.ctx);
    auto unsplit = [](const _Float16* x, int o) {  // x1 + 2^-11 x2 of 4 halves at o
        const f16x4 a = *reinterpret_cast<const f16x4*>(x + o), b = *reinterpret_cast<const f16x4*>(x + o + kPlane);
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (float)a[j] + (float)b[j] * kLoScale;
        return v;
    };
    // LN2 backward: sm.h -> df planes in sm.ctx
    HPre<2> pa = hprefetch<2>(PT, sW2, D, 16 * wv, 0);
    LnBwdPre lnp;
    if (ln2_pre) lnp = *ln2_pre;
    else ln_bwd_load(lnp, io.xhat2, io.rstd2, P + kOffs.o[layer_param(trunk, layer, N2W)], qtok0, b0, last, qtok1);
    ln_bwd_lds(sm.h, sm.ctx, lnp, io.df, io.ln2_part + (size_t)blk * 2 * D, bias + kBiasL2, qtok0, b0, last,
               sm.big, qtok1);
    BTR(TB + 1);
    __syncthreads();
    BTR(TB + 2);
    // du = relu'(u) (W2^T df): wave wv owns hidden tiles 16 wv (-> big planes) and 128 + 16 wv (-> h planes)
    HPre<2> pb;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int row = 128 * t + 16 * wv;
        f32x4 hi[CTQ], lo[CTQ], uu[CTQ];
#pragma unroll
        for (int ct = 0; ct < CTQ; ++ct)
            uu[ct] = ld4(io.u + (size_t)orow(qtok0 + 16 * ct + i16, b0, last) * FF + row + 4 * g);
        zero(hi);
        zero(lo);
        if (t == 0) {
            hgemm_tile<CTQ, 2>(hi, lo, pa, PT, sW2, D, row, 0, cp, qtok0);
            pb = hprefetch<2>(PT, sW2, D, 128 + 16 * wv, 0);
        } else {
            hgemm_tile<CTQ, 2>(hi, lo, pb, PT, sW2, D, row, 0, cp, qtok0);
            pa = hprefetch<2>(PT, sW1, FF, 16 * wv, 0);
        }
        _Float16* dstp = t ? hp : bp;
        f32x4 sd = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ct = 0; ct < CTQ; ++ct) {
            const int tok = qtok0 + 16 * ct + i16;
            const size_t r = (size_t)orow(tok, b0, last);
            const f32x4 u = uu[ct];
            f32x4 d = hi[ct] + lo[ct] * kLoScale;
            d.x = u.x > 0.f ? d.x : 0.f; d.y = u.y > 0.f ? d.y : 0.f;
            d.z = u.z > 0.f ? d.z : 0.f; d.w = u.w > 0.f ? d.w : 0.f;
            *reinterpret_cast<f32x4*>(io.du + r * FF + row + 4 * g) = d;
            hsplit_store(dstp, psw(tok, fo), d);
            sd += d;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) sd[e] = row16_sum(sd[e]);
        if (i16 == 0) st4(bias + kBiasL1 + row + 4 * g, sd);
    }
    BTR(TB + 3);
    __syncthreads();
    BTR(TB + 4);
    // dh1 = df + W1^T du (K = 256: hidden 0-127 in big, 128-255 in h) -> sm.ctx in fp32, after every
    // lane has read its df (the fp32 rows overlap the planes)
    {
        f32x4 hi[CTQ], lo[CTQ];
        zero(hi);
        zero(lo);
        hgemm_tile<CTQ, 2>(hi, lo, pa, PT, sW1, FF, 16 * wv, 0, bp, qtok0);
        hgemm_tile<CTQ, 2>(hi, lo, hprefetch<2>(PT, sW1, FF, 16 * wv, 128), PT, sW1, FF, 16 * wv, 128, hp, qtok0);
#pragma unroll
        for (int ct = 0; ct < CTQ; ++ct) hi[ct] = hi[ct] + lo[ct] * kLoScale + unsplit(cp, psw((qtok0 + 16 * ct + i16), fo));
        __syncthreads();
#pragma unroll
        for (int ct = 0; ct < CTQ; ++ct) st4(sm.ctx + (qtok0 + 16 * ct + i16) * LDH + fo, hi[ct]);
    }
    pa = hprefetch<2>(PT, sWo, D, 16 * wv, 0);
    ln_bwd_load(lnp, io.xhat1, io.rstd1, P + kOffs.o[layer_param(trunk, layer, N1W)], qtok0, b0, last, qtok1);
    AttnPre ap;
    attn_bwd_load<last>(ap, io.qkv, 0, b0, qsel);
    // the position-split modes have no W_in^T GEMM to hide chunk 1's Q / K / V rows behind: both
    // chunks' rows are loaded here (K6 loads chunk 1's behind chunk 0's weight loads, below)
    BTR(TB + 5);
    __syncthreads();
    BTR(TB + 6);
    // LN1 backward: sm.ctx -> dz1 planes in sm.h
    ln_bwd_lds(sm.ctx, sm.h, lnp, io.dz1, io.ln1_part + (size_t)blk * 2 * D, bias + kBiasOut, qtok0, b0, last,
               sm.big, qtok1);
    BTR(TB + 7);
    __syncthreads();
    BTR(TB + 8);
    // d(attention output) = Wo^T dz1 -> sm.ctx (fp32: the attention backward's operand)
    {
        f32x4 hi[CTQ], lo[CTQ];
        zero(hi);
        zero(lo);
        hgemm_tile<CTQ, 2>(hi, lo, pa, PT, sWo, D, 16 * wv, 0, hp, qtok0);
#pragma unroll
        for (int ct = 0; ct < CTQ; ++ct) st4(sm.ctx + (qtok0 + 16 * ct + i16) * LDH + fo, hi[ct] + lo[ct] * kLoScale);
    }
    BTR(TB + 9);
    __syncthreads();
    BTR(TB + 10);
    // attention backward per chunk of 4 heads, dh_in += W_in^T [dq | dk | dv] of the chunk (K = 3 x 64)
    f32x4 hi[S], lo[S];
    zero(hi);
    zero(lo);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        [[maybe_unused]] HPre<2> pw;
        if constexpr (MODE == kBwdFull) pw = hprefetch<2>(PT, sWin, 3 * D, 16 * wv, 64 * c);
        attn_bwd_chunk<last>(sm, ap, c, sm.scr, qsel, io.dqkv, b0, MODE == kBwdPos ? kvc : nullptr, blk);
        __syncthreads();
        BTR(TB + 11 + 2 * c);
        if (tid_x() < 3 * 64) {  // in_proj bias partial of the chunk: the 8 wave rows of sm.scr
            const int i = tid_x();
            float v = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) v += sm.scr[w * 192 + i];
            bias[kBiasIn + (i >> 6) * D + 64 * c + (i & 63)] = v;
        }
        if constexpr (MODE != kBwdFull) {  // the per-position kernels form dL/d(layer input)
            if (c == 0) attn_bwd_load<last>(ap, io.qkv, 1, b0, qsel);
            if (c == 0) __syncthreads();  // sm.scr is rewritten by chunk 1
            continue;
        }
        const HPre<2> pw1 = hprefetch<2>(PT, sWin, 3 * D, 16 * wv, D + 64 * c);
        const HPre<2> pw2 = hprefetch<2>(PT, sWin, 3 * D, 16 * wv, 2 * D + 64 * c);
        if (last) {  // dq is zero outside the query tile: W_in,q^T dq only for column tile 4
            f32x4 h1[1] = {hi[S - 1]}, l1[1] = {lo[S - 1]};
            hgemm_tile<1, 2, 2, kLdbP, kPlaneB>(h1, l1, pw, PT, sWin, 3 * D, 16 * wv, 64 * c, bp, (S - 1) * SPW);
            hi[S - 1] = h1[0];
            lo[S - 1] = l1[0];
        } else {
            hgemm_tile<S, 2, 2, kLdbP, kPlaneB>(hi, lo, pw, PT, sWin, 3 * D, 16 * wv, 64 * c, bp, 0);
        }
        hgemm_tile<S, 2, 2, kLdbP, kPlaneB>(hi, lo, pw1, PT, sWin, 3 * D, 16 * wv, D + 64 * c, bp + 64, 0);
        hgemm_tile<S, 2, 2, kLdbP, kPlaneB>(hi, lo, pw2, PT, sWin, 3 * D, 16 * wv, 2 * D + 64 * c, bp + 128, 0);
        if (c == 0) attn_bwd_load<last>(ap, io.qkv, 1, b0, qsel);  // behind every weight load of the chunk
        if (c == 0) __syncthreads();  // big is rewritten by chunk 1
        BTR(TB + 12 + 2 * c);
    }
    if constexpr (MODE != kBwdFull) return;
    if (layer == 0 && ep) embed_bwd_load(*ep, e_emb, xg, b0);
    next_load();
    // + dz1 on the rows that carried the residual -> sm.h (fp32, after every lane has read its dz1)
    f32x4 res[S];
#pragma unroll
    for (int ct = 0; ct < S; ++ct) {
        const int tok = 16 * ct + i16;
        res[ct] = tok >= qtok0 ? unsplit(hp, psw(tok, fo)) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
#pragma unroll
    for (int ct = 0; ct < S; ++ct) st4(sm.h + (16 * ct + i16) * LDH + fo, hi[ct] + lo[ct] * kLoScale + res[ct]);
    __syncthreads();
    BTR(TB + 15);
}
// K6 and K7's B1 / B2 call bwd_layer through this forwarder, which carries the defaults and the
// layer's first trace stamp. As layer_tail_fwd, the extra call level only fixes the inlining nesting:
// the code objects of k_policy_backward, k_ps_b1 and k_ps_b2 depend on it (called directly: the same
// instructions in another order). Fold it away only together with a same-box benchmark of them.
template <int trunk, int layer, bool last, int TB, class F = NoHook, int MODE = kBwdFull>
__device__ void bwd_layer_fwd(Smem& sm, const float* __restrict__ P, const float* __restrict__ PT, const BwdLayerIO& io,
                              int b0, EmbBwdPre* ep = nullptr, const float* e_emb = nullptr, const float* xg = nullptr,
                              const LnBwdPre* ln2_pre = nullptr, F next_load = F{}, int qt = 0, int prow = -1,
                              float* __restrict__ kvc = nullptr) {
    BTR(TB);
    bwd_layer<trunk, layer, last, TB, F, MODE>(sm, P, PT, io, b0, ep, e_emb, xg, ln2_pre, next_load, qt, prow, kvc);
}

// Embedding backward from sm.h = dL/d(h0) (80 tokens): h0 = relu(We x + be) + pos. Thread =
// (feature, token group of 20); partials reduced over the 4 groups through sm.big -> part [2560]
// in the parameters' order (pos | We | be).
__device__ void embed_bwd(Smem& sm, const EmbBwdPre& ep, float* __restrict__ part, int tb = 55) {
    const int f = tid_x() & (D - 1), grp = tid_x() >> 7;
    if (tid_x() < TOK * LDX / 4) st4(sm.x + 4 * tid_x(), ep.xv);  // input windows (sm.x was scratch)
    __syncthreads();
    BTR(tb);
    float acc[IN + 1 + S];
#pragma unroll
    for (int v = 0; v < IN + 1 + S; ++v) acc[v] = 0.f;
#pragma unroll
    for (int i = 0; i < TOK / 4; ++i) {
        const int tok = grp + 4 * i;  // position tok / 16 = i / 4
        const float gv = sm.h[tok * LDH + f];
        acc[IN + 1 + i / 4] += gv;
        const float gp = ep.ev[i] > 0.f ? gv : 0.f;
        acc[IN] += gp;
        float xr[LDX];  // the token's window row: 4 broadcast b128 reads
#pragma unroll
        for (int q = 0; q < LDX / 4; ++q) {
            const f32x4 x4 = ld4(sm.x + tok * LDX + 4 * q);
            xr[4 * q] = x4.x; xr[4 * q + 1] = x4.y; xr[4 * q + 2] = x4.z; xr[4 * q + 3] = x4.w;
        }
#pragma unroll
        for (int k = 0; k < IN; ++k) acc[k] += gp * xr[k];
    }
    constexpr int NV = IN + 1 + S;  // 20
#pragma unroll
    for (int v = 0; v < NV; ++v) sm.big[(grp * NV + v) * D + f] = acc[v];
    __syncthreads();
    BTR(tb + 1);
    for (int o = tid_x(); o < NV * D; o += NTHR) {
        const int v = o >> 7, ff = o & (D - 1);
        const float s = (sm.big[v * D + ff] + sm.big[(NV + v) * D + ff]) +
                        (sm.big[(2 * NV + v) * D + ff] + sm.big[(3 * NV + v) * D + ff]);
        // state_dict order of the trunk's first parameters: pos [5][128] | We [128][14] | be [128]
        const int dst = v < IN ? S * D + ff * IN + v : (v == IN ? S * D + D * IN + ff : (v - IN - 1) * D + ff);
        part[dst] = s;
    }
}

// Loss gradients of ppo.py:148-169 per sample (torch's min / max / clamp backward conventions:
// ties send half the gradient to each side, clamp passes it on the closed interval), then the
// heads' backward: dz = relu'(z) (W2^T g) for both heads -> io.dz, LDS (actor: sm.z, critic:
// sm.ctx + 64, both [16][LDZ]), and the head.2 weight / bias partials of the 16 samples.
// role (trunk split): 0 both heads, 1 the actor head only, 2 the critic head only.
__device__ void heads_bwd(Smem& sm, const float* __restrict__ P, const BwdIO& io, int b0, int role) {
    const int blk = b0 / SPW;
    float* gs = sm.ctx;                  // [16][4]: dlogit0, dlogit1, dvalue
    float* dzc = sm.ctx + 64;            // critic dz rows
    float* zs = sm.big;                  // relu(head.0) rows of both heads [2][16][64]
    const float inv = 1.0f / (float)io.Bg;
    // the gradient path's 1/Bg pre-scaled by the power of two io.gscale (BwdIO::gscale): gradients
    // leave this function gscale x the loss's, bit for bit (power-of-two scaling commutes with every
    // rounding), and stay that way through the linear backward until k_reduce_grads' 1/gscale
    const float ginv = inv * io.gscale;
    // the critic's gradients additionally x 2^-k (k > 0 only when a value error of the minibatch
    // reaches 16): its per-sample gradient is ~ |v - R|, which returns of configs[4]'s scale and
    // beyond would carry past fp16's range in the split-product dX GEMMs. Every workgroup forms the
    // same k from the forward's per-block maxima (vpart); the critic's reductions undo it
    // (k_reduce_grads reads 2^k from gsc_out).
    // Every wave reduces the maxima itself (a few L2-resident loads per lane), so ck / ginv_c are the
    // same in every lane of the workgroup (wave 0 alone had them). ck saturates at 124
    // for an infinite maximum (2^-124 is still a normal float; a NaN maximum keeps ck = 0: the loss is
    // NaN then anyway).
    float vmx = 0.f;
    for (int i = tid_x() & 63; i < io.nvpart; i += 64) vmx = fmaxf(vmx, io.vpart[i]);
    vmx = wave_max(vmx);
    int vexp = 0;
    (void)frexpf(vmx, &vexp);
    const int ck = !(vmx >= 16.f) ? 0 : vmx < 3.0e38f ? vexp - 4 : 124;  // vmx 2^-ck in [8, 16)
    const float ginv_c = ginv * ldexpf(1.0f, -ck);
    if (tid_x() == 0 && blk == 0 && role != 1 && io.gsc_out) io.gsc_out[0] = ldexpf(1.0f, ck);
    // the four loss sums (used by wave 0 only): from the all-reduced buffer, or summed here from
    // the forward's workgroup partials with k_loss_sums' exact order (train.hip)
    // every global input issued before the first use: z rows (one float4 per thread), the head.2
    // weights of this thread's hidden unit j = tid % 64 (the dz loop below), the per-sample rows,
    // then the loss-sum partials four rows per thread at a time (a dependent chain of L2 round trips
    // before: the heads prologue took 10.7 k cycles of K6)
    const int zt = tid_x() >> 8, zp = (tid_x() >> 4) & 15, zq = tid_x() & 15;
    const f32x4 zr = ld4(io.z[zt] + (size_t)(b0 + zp) * HID + 4 * zq);
    const int jj = tid_x() % HID;
    const float* W2a = P + kOffs.o[kActorHead + 2];
    const float w2a0 = W2a[jj], w2a1 = W2a[HID + jj], w2c = P[kOffs.o[kCriticHead + 2] + jj];
    f32x4 oa = {0.f, 0.f, 0.f, 0.f}, ob = oa;
    if (tid_x() < SPW) {
        oa = ld4(io.smp + (size_t)(b0 + tid_x()) * 8);
        ob = ld4(io.smp + (size_t)(b0 + tid_x()) * 8 + 4);
    }
    // the scheduled values (BwdIO::hyper), with the other global inputs of the prologue
    const float eps_clip = hyper_f32(io.hyper, UAVHIP_HP_EPS_CLIP, io.eps_clip);
    const float entropy_coef = hyper_f32(io.hyper, UAVHIP_HP_ENTROPY_COEF, io.entropy_coef);
    float tot0, tot1, tot2, tot3;
    if (io.fpart) {
        f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
        if (tid_x() < 64) {  // row i's four sums, rows in k_loss_sums' order per lane
#pragma unroll 4
            for (int i = tid_x(); i < io.nfpart; i += 64) s4 += ld4(io.fpart + (size_t)i * 4);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                s4[c] = add_xor32(add_xor16(add_ror8(add_ror4(add_xor2(add_xor1(s4[c]))))));
            if (blk == 0 && role != 2 && tid_x() == 0 && io.tot_out)
                for (int c = 0; c < 4; ++c) io.tot_out[c] = s4[c];
        }
        tot0 = s4[0]; tot1 = s4[1]; tot2 = s4[2]; tot3 = s4[3];
    } else {
        tot0 = io.tot[0]; tot1 = io.tot[1]; tot2 = io.tot[2]; tot3 = io.tot[3];
    }
    BTR(59);
    st4(zs + (zt * SPW + zp) * HID + 4 * zq, zr);
    if (tid_x() < SPW) {
        const int p = tid_x();
        const float o[8] = {oa.x, oa.y, oa.z, oa.w, ob.x, ob.y, ob.z, ob.w};
        const int act = o[0] > 0.f;
        const bool pad = o[0] < 0.f;  // padding row (idx < 0): zero output gradients
        const CatVals c = categorical(o[5], o[6]);
        const float logp = act ? c.lc1 : c.lc0;
        const float ratio = expf(logp - o[1]);
        const float A = o[4], lo = 1.f - eps_clip, hi = 1.f + eps_clip;
        const float s1 = ratio * A;
        const float s2 = fminf(fmaxf(ratio, lo), hi) * A;
        const float gmin = -ginv;  // d(-mean(min)) / d min_i (x gscale)
        const float g1 = s1 < s2 ? gmin : (s1 == s2 ? 0.5f * gmin : 0.f);
        const float g2 = s2 < s1 ? gmin : (s1 == s2 ? 0.5f * gmin : 0.f);
        const float gr = g1 * A + ((ratio >= lo && ratio <= hi) ? g2 * A : 0.f);
        const float glogp = gr * ratio;
        const float gent = -entropy_coef * ginv;
        // back through lc = log(clamp(p)), ent = -sum(lc * p), p = y / s, s = y0 + y1, y = softmax
        float glc0 = -gent * c.p0, glc1 = -gent * c.p1;
        if (act) glc1 += glogp; else glc0 += glogp;
        const float eps = 1.1920928955078125e-07f;
        const float gp0 = -gent * c.lc0 + ((c.p0 >= eps && c.p0 <= 1.f - eps) ? glc0 / c.c0 : 0.f);
        const float gp1 = -gent * c.lc1 + ((c.p1 >= eps && c.p1 <= 1.f - eps) ? glc1 / c.c1 : 0.f);
        const float gsum = -(gp0 * c.y0 + gp1 * c.y1) / (c.s * c.s);
        const float gy0 = gp0 / c.s + gsum, gy1 = gp1 / c.s + gsum;
        const float dot = gy0 * c.y0 + gy1 * c.y1;
        // value: 0.5 * max(mean((v-R)^2), mean((vc-R)^2))
        const float L1 = tot1 * inv, L2 = tot2 * inv;
        const float v = o[7], R = o[3], ov = o[2];
        const float dv = v - ov;
        const float vc = ov + fminf(fmaxf(dv, -eps_clip), eps_clip);
        const float w1 = L1 > L2 ? 1.f : (L1 == L2 ? 0.5f : 0.f);
        const float w2 = L2 > L1 ? 1.f : (L1 == L2 ? 0.5f : 0.f);
        gs[4 * p + 0] = pad ? 0.f : c.y0 * (gy0 - dot);
        gs[4 * p + 1] = pad ? 0.f : c.y1 * (gy1 - dot);
        gs[4 * p + 2] = pad ? 0.f : io.value_coef * (w1 * 2.f * (v - R) * ginv_c +
                                         ((dv >= -eps_clip && dv <= eps_clip) ? w2 * 2.f * (vc - R) * ginv_c : 0.f));
        if (p == 0 && blk == 0 && role != 2 && io.stats) {
            io.stats[0] += (double)(-tot0 * inv);
            io.stats[1] += (double)fmaxf(L1, L2);
            io.stats[2] += (double)(tot3 * inv);
            io.stats[3] += 1.0;
        }
    }
    __syncthreads();
    BTR(60);
    static_assert(NTHR % HID == 0, "dz loop: j = tid % 64 for every i");
    for (int i = tid_x(); i < 2 * SPW * HID; i += NTHR) {
        const int trunk = i / (SPW * HID), p = (i / HID) % SPW, j = i % HID;
        if (role == 1 + (trunk ^ 1)) continue;  // the other role's head
        const float z = zs[(trunk * SPW + p) * HID + j];
        const float g = trunk ? w2c * gs[4 * p + 2] : w2a0 * gs[4 * p] + w2a1 * gs[4 * p + 1];
        const float dz = z > 0.f ? g : 0.f;
        io.dz[trunk][(size_t)(b0 + p) * HID + j] = dz;
        (trunk ? dzc : sm.z)[p * LDZ + j] = dz;
    }
    __syncthreads();
    BTR(61);
    // head.0 bias partials (sum over the 16 samples of dz, from LDS)
    if (tid_x() < 2 * HID && role != 1 + (tid_x() / HID ^ 1)) {
        const int trunk = tid_x() / HID, j = tid_x() % HID;
        const float* d = trunk ? dzc : sm.z;
        float acc = 0.f;
        for (int p = 0; p < SPW; ++p) acc += d[p * LDZ + j];
        io.hpart[(size_t)blk * kHeadPart + kHeadB0 + tid_x()] = acc;
    }
    // head.2 partials, summed over the 16 samples in order: dW2[o][j] = sum g_o z_j, db2[o] = sum g_o
    // [0, 2 HID + 2): actor head.2, [2 HID + 2, 3 HID + 3): critic head.2, then padding (actor role)
    if (tid_x() < kHeadB0 && role != ((tid_x() >= 2 * HID + 2 && tid_x() < 3 * HID + 3) ? 1 : 2)) {
        const int i = tid_x();
        float acc = 0.f;
        if (i < 2 * HID) {
            const int o = i / HID, j = i % HID;
            for (int p = 0; p < SPW; ++p) acc += gs[4 * p + o] * zs[p * HID + j];
        } else if (i < 2 * HID + 2) {
            for (int p = 0; p < SPW; ++p) acc += gs[4 * p + i - 2 * HID];
        } else if (i < 3 * HID + 2) {
            const int j = i - 2 * HID - 2;
            for (int p = 0; p < SPW; ++p) acc += gs[4 * p + 2] * zs[(SPW + p) * HID + j];
        } else if (i < 3 * HID + 3) {
            for (int p = 0; p < SPW; ++p) acc += gs[4 * p + 2];
        }
        io.hpart[(size_t)blk * kHeadPart + i] = acc;
    }
}

// dL/d(trunk output) of the 16 samples = head.0^T dz (MFMA, K = 64; one 16-feature tile per
// wave) -> sm.h rows of column tile 4, the top gradient of the trunk's last layer.
__device__ __forceinline__ void head_input_grad(Smem& sm, const float* __restrict__ W0T, const float* dz) {
    const int wv = tid_x() >> 6, l = lane_id(), i16 = l & 15, g = l >> 4;
    f32x4 acc[1];
    zero(acc);
    gemm_tile<1, 4, 4>(acc, prefetch<4>(W0T, HID, 16 * wv, 0), W0T, HID, 16 * wv, 0, dz, LDZ, 0);
    st4(sm.h + ((S - 1) * SPW + i16) * LDH + 16 * wv + 4 * g, acc[0]);
}

__global__ __launch_bounds__(NTHR) void k_policy_backward(const float* __restrict__ P, const float* __restrict__ PT,
                                                          const BwdIO io) {
    __shared__ __attribute__((aligned(16))) Smem sm;
    // the younger half (waves 4-7, the arbitration loser of every phase) at priority 1
    if (tid_x() >= NTHR / 2) __builtin_amdgcn_s_setprio(1);
    // trunk split (BwdIO::split): workgroups [0, split) the actor head + trunk, then the critic's
    int blk = blockIdx.x, role = 0;
    if (io.split) {
        role = blk < io.split ? 1 : 2;
        if (role == 2) blk -= io.split;
    }
    const int b0 = blk * SPW;
    if (tid_x() < SPW * S) sm.mask[tid_x()] = io.mask[(size_t)b0 * S + tid_x()] != 0.f;
    BTR(0);
    heads_bwd(sm, P, io, b0, role);
    __syncthreads();
    BTR(1);
    // Trunk order (BwdIO::mix): the actor and critic trunks are independent below the heads, so
    // every other group of 8 workgroups (one per XCD) runs the actor first: at any time half the
    // chip is in the other trunk's phases, and the HBM-heavy phases of one overlap the compute of
    // the other instead of all 256 workgroups streaming at once. The critic's dz rows (sm.ctx + 64,
    // clobbered by the actor's layer) come back from io.dz[1], which heads_bwd wrote with them.
    const bool actor_first = role == 0 && io.mix && ((blk >> 3) & 1);
    // actor: head.0, layer 0 (pruned), embedding (twice in the code, once per order: a loop over
    // the two trunks let LICM keep weight prefetches live across both and spilled 578 VGPRs)
    auto actor = [&] {
        head_input_grad(sm, PT + kHeadT, sm.z);
        __syncthreads();
        BTR(53);
        EmbBwdPre ep;
        bwd_layer_fwd<kActorTrunk, 0, true, 36, NoHook, kBwdFull>(sm, P, PT, io.L[0], b0, &ep, io.e[0], io.xg);
        embed_bwd(sm, ep, io.epart + (size_t)blk * 2 * kEmbPart, 57);
        BTR(54);
    };
    if (actor_first) {
        actor();
        __syncthreads();  // the critic's trunk reuses every buffer
        float* dzc = sm.ctx + 64;
        for (int i = tid_x(); i < SPW * HID; i += NTHR)
            dzc[(i / HID) * LDZ + i % HID] = io.dz[1][(size_t)(b0 + i / HID) * HID + i % HID];
        __syncthreads();
    }
    if (role != 1) {  // critic: head.0, layer 1 (pruned), layer 0, embedding
        head_input_grad(sm, PT + kHeadT + D * HID, sm.ctx + 64);
        __syncthreads();
        BTR(2);
        // layer 0's LN2-backward operands are loaded at the end of layer 1's backward
        LnBwdPre l2;
        auto hook = [&] {
            ln_bwd_load(l2, io.L[1].xhat2, io.L[1].rstd2, P + kOffs.o[layer_param(kCriticTrunk, 0, N2W)], 0, b0, false);
        };
        bwd_layer_fwd<kCriticTrunk, 1, true, 4, decltype(hook), kBwdFull>(sm, P, PT + 2 * kLayerT, io.L[2], b0,
                                                                          nullptr, nullptr, nullptr, nullptr, hook);
        EmbBwdPre ep;
        bwd_layer_fwd<kCriticTrunk, 0, false, 20, NoHook, kBwdFull>(sm, P, PT + 1 * kLayerT, io.L[1], b0, &ep,
                                                                    io.e[1], io.xg, &l2);
        embed_bwd(sm, ep, io.epart + ((size_t)blk * 2 + 1) * kEmbPart);
        __syncthreads();
        BTR(52);
    }
    if (role != 2 && !actor_first) actor();
}

// ================================================================== K7: position-split training step
// Small minibatches leave most CUs idle in the 16-samples-per-workgroup kernels above (minibatch 64:
// 8 workgroups, each with ~30 MFLOP of its critic trunk = ~48 us at one CU's MFMA peak). Here every
// full (unpruned) encoder layer runs as 5 workgroups per 16-sample block, one per window position
// (16 tokens = one MFMA column tile): token-local work (embedding, Q|K|V projection, out-projection,
// LayerNorms, FFN) splits exactly; attention needs every position's K / V, so the launches are cut
// there and the K / V rows go through the workspace (L2-resident at these sizes):
//   F1  block x trunk x position: gather, embedding, layer-0 Q|K|V of the position
//   F2  block x (critic x 5 positions | actor x position 4): layer-0 attention for the position's
//       queries, out-proj + LN1 + FFN + LN2; critic: layer-1 K|V of the position (Q at position 4);
//       actor: the head
//   F3  block (critic): layer 1 (pruned: position 4) attention + tail + head, the loss partials
//   B1  block x trunk: loss / head backward, the pruned top layer's backward down to its dqkv rows
//   B2  block x trunk x position: dL/d(top layer input) at the position = W_in^T dqkv + residual;
//       actor: embedding backward; critic: layer-0 backward for the position's queries -- its dq rows
//       and its share of every position's dk / dv (kvc)
//   B3  block x position (critic): dk / dv of the position = the 5 shares in position order (fixed:
//       deterministic), W_in^T, residual, embedding backward
// Partial rows (bias / LayerNorm / embedding gradients) are per (block, position): row b * 5 + s
// (per-block layers use row b * 5). The same weight-gradient GEMM, reduction and Adam follow.
constexpr int LDQ = 3 * D + 8;  // a [dq | dk | dv] row in LDS (392 floats: 2 mod 16 slots of 16 B)

__device__ __forceinline__ void ps_mask(Smem& sm, const float* __restrict__ mask, int b0) {
    if (tid_x() < SPW * S) sm.mask[tid_x()] = mask[(size_t)b0 * S + tid_x()] != 0.f;
}

// Workspace rows [(b0 + p) * 5 + s][c0 .. c0 + cols) -> LDS rows s * 16 + p (stride lds)
__device__ __forceinline__ void ps_rows_in(float* dst, int lds, const float* __restrict__ src, int ld, int c0, int cols,
                                           int s, int b0) {
    const int n4 = cols / 4;
    for (int i = tid_x(); i < SPW * n4; i += NTHR) {
        const int p = i / n4, q = i - p * n4;
        st4(dst + (s * SPW + p) * lds + 4 * q, ld4(src + (size_t)trow(s * SPW + p, b0) * ld + c0 + 4 * q));
    }
}

// Embedding of window position s (transformer_net.py:57-59): h = relu(W_e x + b_e) + pos[s] -> sm.h
// rows 16 s + p, the planes of h into sm.ctx (ps_inproj's operand) and the e / h0 workspace rows;
// wave w computes features [16 w, 16 w + 16).
// The embedding's global operands (ps_embed_load: issued by k_ps_f1 before the window gather).
struct PsEmbPre {
    f32x4 a, bb, pp;
};
__device__ __forceinline__ PsEmbPre ps_embed_load(const float* __restrict__ P, int trunk, int s) {
    const float* We = P + kOffs.o[trunk + EMB_W];
    const int l = lane_id(), i16 = l & 15, g = l >> 4, wv = tid_x() >> 6;
    const int f = 16 * wv + i16;
    PsEmbPre r;
    r.a.x = 4 * g + 0 < IN ? We[f * IN + 4 * g + 0] : 0.f;
    r.a.y = 4 * g + 1 < IN ? We[f * IN + 4 * g + 1] : 0.f;
    r.a.z = 4 * g + 2 < IN ? We[f * IN + 4 * g + 2] : 0.f;
    r.a.w = 4 * g + 3 < IN ? We[f * IN + 4 * g + 3] : 0.f;
    r.bb = ld4(P + kOffs.o[trunk + EMB_B] + 16 * wv + 4 * g);
    r.pp = ld4(P + kOffs.o[trunk + POS] + s * D + 16 * wv + 4 * g);
    return r;
}
__device__ void ps_embed(Smem& sm, const PsEmbPre& ep, float* __restrict__ e_out, float* __restrict__ h_out, int b0,
                         int s, int ti) {
    const int l = lane_id(), i16 = l & 15, g = l >> 4, wv = tid_x() >> 6;
    const f32x4 a = ep.a, bb = ep.bb, pp = ep.pp;
    const f32x4 x = ld4(sm.x + (s * SPW + i16) * LDX + 4 * g);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], x[j], acc, 0, 0, 0);
    f32x4 e = acc + bb;
    e.x = fmaxf(e.x, 0.f); e.y = fmaxf(e.y, 0.f); e.z = fmaxf(e.z, 0.f); e.w = fmaxf(e.w, 0.f);
    const f32x4 v = e + pp;
    st4(sm.h + (s * SPW + i16) * LDH + 16 * wv + 4 * g, v);
    // scaled per token (its window row's range)
    hsplit_store(reinterpret_cast<_Float16*>(sm.ctx), psw((s * SPW + i16), 16 * wv + 4 * g),
                 v * e_sc_v(sm.rtab[kRtE + 2 * ti], sm.rtab[kRtE + 2 * ti + 1], sm.tmax[s * SPW + i16]).sc);
    const size_t r = (size_t)trow(s * SPW + i16, b0);
    st4(e_out + r * D + 16 * wv + 4 * g, e);
    st4(h_out + r * D + 16 * wv + 4 * g, v);
}

// in_proj rows [16 tile0, 384) of the 16 tokens of position s -> qkv rows (Q = rows 0-127, K = 128-255,
// V = 256-383 of a [b * 5 + s][384] row), bias added, as split products: the operand planes of the 16
// tokens at X rows 16 s + p, W's split copy at soff.
// Every weight block and bias of the wave's (at most 3) row tiles is loaded in one round
// (ps_inproj_load, which a caller issues ahead of the operand's producer): one exposed L2 round trip
// instead of one per tile -- the same MFMA sequence per tile, so the same sums.
constexpr int kPsInTiles = 3;  // row tiles per wave: 24 tiles of in_proj over 8 waves
struct PsInPre {
    HPre<4> w[kPsInTiles];
    f32x4 bb[kPsInTiles];
};
__device__ __forceinline__ void ps_inproj_load(PsInPre& r, const float* __restrict__ P, int soff,
                                               const float* __restrict__ bias, int tile0) {
    const int g = lane_id() >> 4, wv = tid_x() >> 6;
#pragma unroll
    for (int k = 0; k < kPsInTiles; ++k) {
        // unconditional loads (a tile below tile0 reloads tile wv: loaded, never used)
        const int t = tile0 + wv + NW * k, row = 16 * (t < 3 * D / 16 ? t : wv);
        r.w[k] = hprefetch<4>(P, soff, D, row, 0);
        r.bb[k] = ld4(bias + row + 4 * g);
    }
}
// inv: 2^s of the operand at this lane's token (the caller's: layer 0 per token, layer 1 static)
__device__ void ps_inproj(const PsInPre& pre, const float* __restrict__ P, int soff, float* __restrict__ qkv,
                                int tile0, int s, int b0, const _Float16* X, float inv) {
    const int l = lane_id(), i16 = l & 15, g = l >> 4, wv = tid_x() >> 6;
    const size_t r = (size_t)trow(s * SPW + i16, b0);
#pragma unroll
    for (int k = 0; k < kPsInTiles; ++k) {
        const int t = tile0 + wv + NW * k;
        if (t >= 3 * D / 16) break;  // wave-uniform
        const int row = 16 * t;
        f32x4 hi[1], lo[1];
        zero(hi);
        zero(lo);
        hgemm_tile<1, 4>(hi, lo, pre.w[k], P, soff, D, row, 0, X, s * SPW);
        st4(qkv + r * 3 * D + row + 4 * g, (hi[0] + lo[0] * kLoScale) * inv + pre.bb[k]);
    }
}
static_assert(NW * kPsInTiles == 3 * D / 16, "ps_inproj_load covers every in_proj row tile");

// Q of position s and K | V of all five positions for the heads of chunk c -> sm.big [tok][Q|K|V];
// in two halves so that chunk 1's loads can be in flight during chunk 0's attention
constexpr int kQkvItems = SPW * 16 + TOK * 32, kQkvIt = (kQkvItems + NTHR - 1) / NTHR;
struct QkvPre {
    f32x4 v[kQkvIt];
};
__device__ __forceinline__ void ps_qkv_item(int i, int s, int& tok, int& part, int& q) {
    if (i < SPW * 16) {
        tok = s * SPW + i / 16; part = 0; q = i % 16;
    } else {
        const int k = i - SPW * 16;
        tok = k / 32; part = 1 + (k % 32) / 16; q = k % 16;
    }
}
__device__ __forceinline__ void ps_qkv_load(QkvPre& r, const float* __restrict__ qkv, int c, int s, int b0) {
#pragma unroll
    for (int k = 0; k < kQkvIt; ++k) {
        const int i = tid_x() + NTHR * k;
        if (i < kQkvItems) {
            int tok, part, q;
            ps_qkv_item(i, s, tok, part, q);
            r.v[k] = ld4(qkv + (size_t)trow(tok, b0) * 3 * D + part * D + 64 * c + 4 * q);
        }
    }
}
__device__ __forceinline__ void ps_qkv_store(Smem& sm, const QkvPre& r, int s) {
#pragma unroll
    for (int k = 0; k < kQkvIt; ++k) {
        const int i = tid_x() + NTHR * k;
        if (i < kQkvItems) {
            int tok, part, q;
            ps_qkv_item(i, s, tok, part, q);
            st4(sm.big + tok * LDB + part * 64 + 4 * q, r.v[k]);
        }
    }
}
// the attention of both chunks (K7 F2 / F3): chunk 1's Q | K | V loads overlap chunk 0's attention
// (the output's planes scaled for layer `layer` of trunk `trunk`)
template <int trunk, int layer>
__device__ __forceinline__ void ps_attention(Smem& sm, const float* __restrict__ qkv, int s, int b0,
                                             const float* __restrict__ P) {
    QkvPre r;
    ps_qkv_load(r, qkv, 0, s, b0);
    ps_qkv_store(sm, r, s);
    __syncthreads();
    ps_qkv_load(r, qkv, 1, s, b0);
    attention_chunk<trunk, layer>(sm, 0, s, 1, P);
    __syncthreads();
    ps_qkv_store(sm, r, s);
    __syncthreads();
    attention_chunk<trunk, layer>(sm, 1, s, 1, P);
    __syncthreads();
}

__global__ __launch_bounds__(NTHR) void k_ps_f1(const float* __restrict__ P, const float* __restrict__ states, int B,
                                                const TrainIO io) {
    __shared__ __attribute__((aligned(16))) Smem sm;
    const int blk = blockIdx.x / 10, r = blockIdx.x % 10, s = r % S, b0 = blk * SPW;
    const bool critic = r >= S;
    const int trunk = critic ? kCriticTrunk : kActorTrunk;
    // the actor's only layer is pruned: Q at position 4 only
    const int tile0 = critic || s == S - 1 ? 0 : D / 16;
    const int soff = critic ? split_slot(layer_param(kCriticTrunk, 0, INW)) : split_slot(layer_param(kActorTrunk, 0, INW));
    // every global operand of the embedding and of the in_proj GEMM first: their L2 round trip
    // overlaps the window gather's
    const PsEmbPre ep = ps_embed_load(P, trunk, s);
    PsInPre wp;
    ps_inproj_load(wp, P, soff, P + kOffs.o[layer_param(trunk, 0, INB)], tile0);
    gather_windows<true>(sm, states, B, io, b0, r == 0, P + kRangeOff);  // one workgroup per block writes the rows
    load_rtab(sm, P);  // behind the gather's loads (its arithmetic waits on nothing they need)
    __syncthreads();
    // the step's derived scales, once: F2 / F3 and the weight-gradient GEMM read them (TrainIO::rtab_out)
    if (blockIdx.x == 0 && tid_x() < kRtN && io.rtab_out) io.rtab_out[tid_x()] = sm.rtab[tid_x()];
    ps_embed(sm, ep, io.e[critic ? 1 : 0], io.h0[critic ? 1 : 0], b0, s, critic ? 1 : 0);
    __syncthreads();
    const float m = sm.tmax[s * SPW + (lane_id() & 15)];
    ps_inproj(wp, P, soff, io.L[critic ? 1 : 0].qkv, tile0, s, b0, reinterpret_cast<const _Float16*>(sm.ctx),
              critic ? e_sc<kCriticTrunk>(sm, m).inv : e_sc<kActorTrunk>(sm, m).inv);
}

__global__ __launch_bounds__(NTHR) void k_ps_f2(const float* __restrict__ P, const TrainIO io) {
    __shared__ __attribute__((aligned(16))) Smem sm;
    const int blk = blockIdx.x / 6, r = blockIdx.x % 6, b0 = blk * SPW, wv = tid_x() >> 6;
    const bool critic = r < S;
    const int s = critic ? r : S - 1, ti = critic ? 1 : 0;
    // the out-projection's first weight blocks ahead of the attention (whose Q | K | V loads and
    // barriers then cover their round trip)
    HPre<2> po;
    po = hprefetch<2>(P, critic ? split_slot(layer_param(kCriticTrunk, 0, OUTW)) : split_slot(layer_param(kActorTrunk, 0, OUTW)),
                      D, 16 * wv, 0);
    // the block's window-row maxima (F1's) first: reduced once the rows below have landed (the
    // vector memory counter retires in order), not waited for ahead of their loads
    const float a0v = a0f_load(io.tmax + (size_t)b0 * S);
    ps_mask(sm, io.mask, b0);
    ps_rows_in(sm.h, LDH, io.h0[ti], D, 0, D, s, b0);  // the layer input (residual) of the position
    load_rtab_ready(sm, io.rtab_out);  // F1's derived table, behind the loads above
    float ec[8];  // layer 0's constants (kRgE .. kRgA0 + 3 = the table's kRtE ..): uniform loads
#pragma unroll
    for (int k = 0; k < 8; ++k) ec[k] = io.rtab_out[kRtE + k];
    const float xm = a0f_finish(sm, a0v, ec, ec + 4);
    if (r == 0 && tid_x() == 0 && io.xmax) io.xmax[blk] = xm;  // the block's range for the weight gradients
    if (critic) ps_attention<kCriticTrunk, 0>(sm, io.L[ti].qkv, s, b0, P);
    else ps_attention<kActorTrunk, 0>(sm, io.L[ti].qkv, s, b0, P);
    APre<4> ph;  // the actor head's weights
    if (critic) {
        // layer 1's in_proj weights and biases are issued before LN2 (the tail's hook), behind
        // every weight load of the tail
        constexpr int s1 = split_slot(layer_param(kCriticTrunk, 1, INW));
        const int tile0 = s == S - 1 ? 0 : D / 16;
        PsInPre wp;
        auto hook = [&] { ps_inproj_load(wp, P, s1, P + kOffs.o[layer_param(kCriticTrunk, 1, INB)], tile0); };
        layer_tail<kCriticTrunk, 0, false, true, decltype(hook), 1>(sm, P, po, io.L[1], b0, hook, s * SPW);
        __syncthreads();
        // layer 1 (pruned) of this position: K | V, and Q at position 4, from LN2's planes in sm.h
        ps_inproj(wp, P, s1, io.L[2].qkv, tile0, s, b0, reinterpret_cast<const _Float16*>(sm.h),
                  op_sc<kCriticTrunk, 0, kOpLn2>(sm).inv);
        return;
    }
    auto hook = [&] {  // the head's weights before LN2
        if (wv < 4) ph = prefetch<4>(P + kOffs.o[kActorHead], D, 16 * wv, 0);
    };
    layer_tail<kActorTrunk, 0, true, true, decltype(hook)>(sm, P, po, io.L[0], b0, hook);
    __syncthreads();
    head_mlp<kActorHead, 2>(sm, P, ph, sm.logits);
    store_hidden(sm, io.z[0], b0);
    if (tid_x() < SPW) {
        float* o = io.smp + (size_t)(b0 + tid_x()) * 8;
        o[5] = sm.logits[2 * tid_x()];
        o[6] = sm.logits[2 * tid_x() + 1];
    }
}

__global__ __launch_bounds__(NTHR) void k_ps_f3(const float* __restrict__ P, const TrainIO io) {
    __shared__ __attribute__((aligned(16))) Smem sm;
    const int b0 = blockIdx.x * SPW, wv = tid_x() >> 6;
    // the out-projection's first weight blocks ahead of the attention (as k_ps_f2)
    HPre<2> po;
    po = hprefetch<2>(P, split_slot(layer_param(kCriticTrunk, 1, OUTW)), D, 16 * wv, 0);
    ps_mask(sm, io.mask, b0);
    ps_rows_in(sm.h, LDH, io.L[1].h2, D, 0, D, S - 1, b0);  // layer 1's input (residual) at position 4
    load_rtab_ready(sm, io.rtab_out);  // F1's derived table, behind the loads above
    ps_attention<kCriticTrunk, 1>(sm, io.L[2].qkv, S - 1, b0, P);
    APre<4> ph;
    auto hook = [&] {  // the head's weights before LN2
        if (wv < 4) ph = prefetch<4>(P + kOffs.o[kCriticHead], D, 16 * wv, 0);
    };
    layer_tail<kCriticTrunk, 1, true, true, decltype(hook), 2>(sm, P, po, io.L[2], b0, hook);  // residual in sm.h: PSX = 2
    __syncthreads();
    head_mlp<kCriticHead, 1>(sm, P, ph, sm.value);
    store_hidden(sm, io.z[1], b0);
    if (tid_x() < SPW) {  // the actor's logits (F2) beside the value: the block's loss partials
        const float* o = io.smp + (size_t)(b0 + tid_x()) * 8;
        sm.logits[2 * tid_x()] = o[5];
        sm.logits[2 * tid_x() + 1] = o[6];
    }
    __syncthreads();
    loss_partials(sm, io, b0);
}

__global__ __launch_bounds__(NTHR) void k_ps_b1(const float* __restrict__ P, const float* __restrict__ PT,
                                                const BwdIO io) {
    __shared__ __attribute__((aligned(16))) Smem sm;
    if (tid_x() >= NTHR / 2) __builtin_amdgcn_s_setprio(1);
    const int blk = blockIdx.x >> 1, role = 1 + (blockIdx.x & 1), b0 = blk * SPW;
    ps_mask(sm, io.mask, b0);
    heads_bwd(sm, P, io, b0, role);
    __syncthreads();
    if (role == 2) {  // critic: head.0, layer 1 (pruned) down to its dqkv rows
        head_input_grad(sm, PT + kHeadT + D * HID, sm.ctx + 64);
        __syncthreads();
        bwd_layer_fwd<kCriticTrunk, 1, true, 4, NoHook, kBwdNoDx>(sm, P, PT + 2 * kLayerT, io.L[2], b0, nullptr, nullptr,
                                                                  nullptr, nullptr, NoHook{}, 0, blk * S);
    } else {  // actor: head.0, layer 0 (pruned) down to its dqkv rows
        head_input_grad(sm, PT + kHeadT, sm.z);
        __syncthreads();
        bwd_layer_fwd<kActorTrunk, 0, true, 36, NoHook, kBwdNoDx>(sm, P, PT, io.L[0], b0, nullptr, nullptr, nullptr,
                                                                  nullptr, NoHook{}, 0, blk * S);
    }
}

// The 16 [dq | dk | dv] rows of position s -> sm.big rows p (stride LDQ); with_q = false: a pruned
// layer off its query position (dq never written there: zero)
// (as the two fp16 planes of ps_dx's split products, both in one row of 2 LDQ halves, plane 2 at
// + 3 D: conflict-free ds_read_b128)
__device__ __forceinline__ void ps_big_store(Smem& sm, int p, int q, const f32x4 v) {
    _Float16* bp = reinterpret_cast<_Float16*>(sm.big);
    f16x4 a, b;
    f16_split4(v, a, b);
    *reinterpret_cast<f16x4*>(bp + p * 2 * LDQ + 4 * q) = a;  // [p][plane 1 | plane 2 | pad]
    *reinterpret_cast<f16x4*>(bp + p * 2 * LDQ + 3 * D + 4 * q) = b;
}
__device__ __forceinline__ void ps_dqkv_in(Smem& sm, const float* __restrict__ dqkv, bool with_q, int s, int b0) {
    for (int i = tid_x(); i < SPW * 96; i += NTHR) {
        const int p = i / 96, q = i - 96 * p;
        f32x4 v = ld4(dqkv + (size_t)trow(s * SPW + p, b0) * 3 * D + 4 * q);
        if (!with_q && q < 32) v = f32x4{0.f, 0.f, 0.f, 0.f};
        ps_big_store(sm, p, q, v);
    }
}
// dL/d(layer input) of position s = W_in^T [dq | dk | dv] (sm.big, ps_dqkv_in) + the residual rows
// res + p * res_ld (nullptr: none) -> sm.h rows 16 s + p. The split GEMM's weights (all three parts,
// every k block: ps_dx_load) are issued by the caller before the [dq | dk | dv] rows are read in, so
// their L2 round trip overlaps that one (one exposed round trip instead of one per part).
struct PsDxPre {
    HPre<4> w[3];
    f32x4 res;  // this lane's residual float4 (zero without a residual)
};
__device__ __forceinline__ void ps_dx_load(PsDxPre& r, const float* __restrict__ WinT, const float* __restrict__ res,
                                           int res_ld) {
    const int l = lane_id(), i16 = l & 15, g = l >> 4, wv = tid_x() >> 6;
#pragma unroll
    for (int part = 0; part < 3; ++part) r.w[part] = hprefetch<4>(WinT, kTSplit, 3 * D, 16 * wv, part * D);
    // unconditional (WinT's first float4 stands in when there is no residual; ps_dx then ignores it)
    r.res = ld4(res ? res + (size_t)i16 * res_ld + 16 * wv + 4 * g : WinT);
}
__device__ void ps_dx(Smem& sm, const PsDxPre& pw, const float* __restrict__ WinT, bool with_q, bool has_res,
                      int s) {
    const int l = lane_id(), i16 = l & 15, g = l >> 4, wv = tid_x() >> 6;
    const int fo = 16 * wv + 4 * g;
    f32x4 acc[1], lo[1];  // WinT + kTSplit: the split copy of this layer's in_proj^T
    zero(acc);
    zero(lo);
    const _Float16* bp = reinterpret_cast<const _Float16*>(sm.big);
#pragma unroll
    for (int part = 0; part < 3; ++part) {
        if (part == 0 && !with_q) continue;
        hgemm_tile<1, 4, 4, 2 * LDQ, 3 * D>(acc, lo, pw.w[part], WinT, kTSplit, 3 * D, 16 * wv, part * D, bp + part * D, 0);
    }
    acc[0] += lo[0] * kLoScale;
    f32x4 v = acc[0];
    if (has_res) v += pw.res;  // (wave-uniform) the residual ps_dx_load read
    st4(sm.h + (s * SPW + i16) * LDH + fo, v);
}

// Embedding backward of position s from sm.h rows 16 s + p = dL/d(h0): thread = (feature, token
// group of 4); the [pos | We | be] partial row of (block, position) -> part (only pos row s nonzero).
// Its global operands (ps_embed_bwd_load, issued by the caller ahead of the W_in^T GEMM): this
// thread's embedding values (the ReLU mask) and one float4 of the position's input rows.
struct PsEmbBwdPre {
    float ev[SPW / 4];
    f32x4 xv;
};
__device__ __forceinline__ void ps_embed_bwd_load(PsEmbBwdPre& r, const float* __restrict__ e,
                                                  const float* __restrict__ xg, int s, int b0) {
    const int f = tid_x() & (D - 1), grp = tid_x() >> 7;
    const int i = tid_x() < SPW * LDX / 4 ? tid_x() : 0;  // unconditional load (threads >= 64: unused)
    const int p = i / (LDX / 4), q = i % (LDX / 4);
    r.xv = ld4(xg + (size_t)trow(s * SPW + p, b0) * 16 + 4 * q);
#pragma unroll
    for (int k = 0; k < SPW / 4; ++k) r.ev[k] = e[(size_t)trow(s * SPW + grp + 4 * k, b0) * D + f];
}
__device__ void ps_embed_bwd(Smem& sm, const PsEmbBwdPre& r, float* __restrict__ part, int s) {
    const int f = tid_x() & (D - 1), grp = tid_x() >> 7;
    if (tid_x() < SPW * LDX / 4) {
        const int p = tid_x() / (LDX / 4), q = tid_x() % (LDX / 4);
        st4(sm.x + p * LDX + 4 * q, r.xv);
    }
    float ev[SPW / 4];
#pragma unroll
    for (int i = 0; i < SPW / 4; ++i) ev[i] = r.ev[i];
    __syncthreads();
    float acc[IN + 1], accp = 0.f;
#pragma unroll
    for (int v = 0; v < IN + 1; ++v) acc[v] = 0.f;
#pragma unroll
    for (int i = 0; i < SPW / 4; ++i) {
        const int p = grp + 4 * i;
        const float gv = sm.h[(s * SPW + p) * LDH + f];
        accp += gv;
        const float gp = ev[i] > 0.f ? gv : 0.f;
        acc[IN] += gp;
#pragma unroll
        for (int q = 0; q < LDX / 4; ++q) {
            const f32x4 x4 = ld4(sm.x + p * LDX + 4 * q);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * q + k < IN) acc[4 * q + k] += gp * x4[k];
        }
    }
    constexpr int NV = IN + 1 + S;  // 20
#pragma unroll
    for (int v = 0; v < NV; ++v)
        sm.big[(grp * NV + v) * D + f] = v <= IN ? acc[v] : (v == IN + 1 + s ? accp : 0.f);
    __syncthreads();
    for (int o = tid_x(); o < NV * D; o += NTHR) {
        const int v = o >> 7, ff = o & (D - 1);
        const float sum = (sm.big[v * D + ff] + sm.big[(NV + v) * D + ff]) +
                          (sm.big[(2 * NV + v) * D + ff] + sm.big[(3 * NV + v) * D + ff]);
        const int dst = v < IN ? S * D + ff * IN + v : (v == IN ? S * D + D * IN + ff : (v - IN - 1) * D + ff);
        part[dst] = sum;
    }
}

__global__ __launch_bounds__(NTHR) void k_ps_b2(const float* __restrict__ P, const float* __restrict__ PT,
                                                const BwdIO io, float* __restrict__ kvc) {
    __shared__ __attribute__((aligned(16))) Smem sm;
    if (tid_x() >= NTHR / 2) __builtin_amdgcn_s_setprio(1);
    const int blk = blockIdx.x / 10, r = blockIdx.x % 10, s = r % S, b0 = blk * SPW, prow = blk * S + s;
    const bool critic = r >= S, q4 = s == S - 1;
    // dL/d(input of the trunk's top, pruned layer) at position s; its residual path (LN1's input
    // gradient, compact [b] rows) exists at the query position 4 only
    const BwdLayerIO& top = io.L[critic ? 2 : 0];
    const float* WinT = PT + (critic ? 2 : 0) * kLayerT + kTWin;
    ps_mask(sm, io.mask, b0);
    ps_dqkv_in(sm, top.dqkv, q4, s, b0);
    __syncthreads();
    // (the GEMM's operands loaded here, not ahead of the dq | dk | dv rows: ahead measured 0.2-0.3 us
    // slower in this kernel, r04x)
    PsDxPre pw;
    ps_dx_load(pw, WinT, q4 ? top.dz1 + (size_t)b0 * D : nullptr, D);
    if (!critic) {  // the actor: the embedding backward's operands ahead of the GEMM
        PsEmbBwdPre eb;
        ps_embed_bwd_load(eb, io.e[0], io.xg, s, b0);
        ps_dx(sm, pw, WinT, q4, q4, s);
        __syncthreads();
        ps_embed_bwd(sm, eb, io.epart + (size_t)prow * 2 * kEmbPart, s);
        return;
    }
    ps_dx(sm, pw, WinT, q4, q4, s);
    __syncthreads();
    bwd_layer_fwd<kCriticTrunk, 0, false, 20, NoHook, kBwdPos>(sm, P, PT + kLayerT, io.L[1], b0, nullptr, nullptr, nullptr,
                                                               nullptr, NoHook{}, s * SPW, prow, kvc);
}

__global__ __launch_bounds__(NTHR) void k_ps_b3(const float* __restrict__ PT, const BwdIO io,
                                                const float* __restrict__ kvc) {
    __shared__ __attribute__((aligned(16))) Smem sm;
    const int blk = blockIdx.x / S, j = blockIdx.x % S, b0 = blk * SPW, prow = blk * S + j;
    // [dq | dk | dv] rows of position j: dq from B2 (position j), dk / dv = the five query
    // positions' shares summed in position order (deterministic); dk / dv -> the dqkv rows
    float* dqkv = io.L[1].dqkv;
    // + LN1's input gradient of layer 0 at position j (the residual path); the GEMM's weights, the
    // residual rows and the embedding backward's operands are loaded ahead of the [dq | dk | dv] rows
    const float* WinT = PT + kLayerT + kTWin;
    PsDxPre pw;
    ps_dx_load(pw, WinT, io.L[1].dz1 + (size_t)trow(j * SPW, b0) * D, S * D);
    PsEmbBwdPre eb;
    ps_embed_bwd_load(eb, io.e[1], io.xg, j, b0);
    for (int i = tid_x(); i < SPW * 96; i += NTHR) {
        const int p = i / 96, q = i - 96 * p, tok = j * SPW + p;
        const size_t row = (size_t)trow(tok, b0);
        f32x4 v;
        if (q < 32) {
            v = ld4(dqkv + row * 3 * D + 4 * q);
        } else {
            v = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < S; ++s) v += ld4(kvc + ((size_t)(blk * S + s) * TOK + tok) * 2 * D + 4 * (q - 32));
            st4(dqkv + row * 3 * D + 4 * q, v);
        }
        ps_big_store(sm, p, q, v);
    }
    __syncthreads();
    ps_dx(sm, pw, WinT, true, true, j);
    __syncthreads();
    ps_embed_bwd(sm, eb, io.epart + ((size_t)prow * 2 + 1) * kEmbPart, j);
}


}  // namespace pol
}  // namespace uavhip

using namespace uavhip;

namespace uavhip {
namespace pol {
int policy_forward_train(const float* packed, const float* states, const TrainIO& io, int Bm, hipStream_t st) {
    hipLaunchKernelGGL(k_policy_forward<true>, dim3((io.split ? 2 : 1) * (Bm / SPW)), dim3(NTHR), 0, st, packed,
                       states, Bm, nullptr, 0ull, 0ull, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, io,
                       RowIO{}, uavhip_env{}, EnvOut{});
    return check_launch("k_policy_forward<train>");
}

int policy_loss_partials(const TrainIO& io, int Bm, hipStream_t st) {
    hipLaunchKernelGGL(k_loss_partials, dim3(Bm / SPW), dim3(64), 0, st, io);
    return check_launch("k_loss_partials");
}

int policy_forward_ps(const float* packed, const float* states, const TrainIO& io, int Bm, hipStream_t st) {
    if (!io.rtab_out) {  // F2 / F3 load F1's derived range table from it
        set_error("policy_forward_ps: TrainIO::rtab_out is NULL");
        return UAVHIP_EINVAL;
    }
    const int nblk = Bm / SPW;
    hipLaunchKernelGGL(k_ps_f1, dim3(nblk * 10), dim3(NTHR), 0, st, packed, states, Bm, io);
    if (const int rc = check_launch("k_ps_f1")) return rc;
    hipLaunchKernelGGL(k_ps_f2, dim3(nblk * 6), dim3(NTHR), 0, st, packed, io);
    if (const int rc = check_launch("k_ps_f2")) return rc;
    hipLaunchKernelGGL(k_ps_f3, dim3(nblk), dim3(NTHR), 0, st, packed, io);
    return check_launch("k_ps_f3");
}

int policy_backward_ps(const float* packed, const float* packedT, const BwdIO& io, float* kvc, int Bm, hipStream_t st) {
    const int nblk = Bm / SPW;
    hipLaunchKernelGGL(k_ps_b1, dim3(nblk * 2), dim3(NTHR), 0, st, packed, packedT, io);
    if (const int rc = check_launch("k_ps_b1")) return rc;
    hipLaunchKernelGGL(k_ps_b2, dim3(nblk * 10), dim3(NTHR), 0, st, packed, packedT, io, kvc);
    if (const int rc = check_launch("k_ps_b2")) return rc;
    hipLaunchKernelGGL(k_ps_b3, dim3(nblk * S), dim3(NTHR), 0, st, packedT, io, static_cast<const float*>(kvc));
    return check_launch("k_ps_b3");
}

int policy_backward_train(const float* packed, const float* packedT, const BwdIO& io, int Bm, hipStream_t st) {
    hipLaunchKernelGGL(k_policy_backward, dim3((io.split ? 2 : 1) * (Bm / SPW)), dim3(NTHR), 0, st, packed, packedT,
                       io);
    return check_launch("k_policy_backward");
}


// flat (state_dict order, plain layout) -> packed (GEMM weights in MFMA fragment order) and, when
// packedT is given, the backward's fp32 transposed copies: the slots of the layers' [in_proj^T |
// out_proj^T | linear1^T | linear2^T] (NaN: the backward reads their split copies, k_policyT_split),
// then head.0^T of both heads, with packedT[((r/16) * K/16 + k/16) * 256 + (r%16 + 16 ((k%16)/4)) * 4
// + k%4] = W[k][r]. One thread per output float4.
__global__ __launch_bounds__(256) void k_policy_pack(const float* __restrict__ flat, float* __restrict__ packed,
                                                     float* __restrict__ packedT) {
    constexpr int nq = kOffs.o[kNumParams] / 4;
    const int i = blockIdx.x * 256 + tid_x();
    if (i < nq) {
        const int f = 4 * i;
        int lo = 0, hi = kNumParams;  // parameter q: kOffs.o[q] <= f < kOffs.o[q + 1]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (f >= kOffs.o[mid]) lo = mid;
            else hi = mid;
        }
        const int local = f - kOffs.o[lo], K = kTileK[lo];
        int src = f;
        if (K != 0 && local < kSizes[lo]) {  // fragment order of [R][K]: float4 = 4 consecutive k
            const int lane = (local >> 2) & 63, blk = local >> 8, KB = K / 16;
            const int kb = blk % KB, rt = blk / KB;
            src = kOffs.o[lo] + (16 * rt + (lane & 15)) * K + 16 * kb + 4 * (lane >> 4);
        }
        // the training pack (packedT given): the training kernels read the layer GEMM weights only
        // through their split copies, so the fp32 copies are filled with NaN (a read would poison
        // every output) and k_adam does not refresh them
        const bool dead = packedT && K != 0 && split_slot(lo) >= 0;
        *reinterpret_cast<f32x4*>(packed + f) =
            dead ? f32x4{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")}
                 : *reinterpret_cast<const f32x4*>(flat + src);
        return;
    }
    if (!packedT || i >= nq + kPackedTFloats / 4) return;
    if (4 * (i - nq) < kHeadT) {  // a layer weight's fp32 transposed copy: never read (NaN, as above)
        *reinterpret_cast<f32x4*>(packedT + 4 * (i - nq)) =
            f32x4{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
        return;
    }
    // head.0 weight [64][128] of the actor / critic head, transposed
    const int idx = 4 * (i - nq);
    const int h = (idx - kHeadT) / (D * HID);
    const int src = kOffs.o[h ? kCriticHead : kActorHead], m = idx - kHeadT - h * D * HID;
    constexpr int Rt = D, Kt = HID;
    const int lane = (m >> 2) & 63, blk = m >> 8, KBt = Kt / 16;
    const int kb = blk % KBt, rt = blk / KBt;
    const int r = 16 * rt + (lane & 15), k = 16 * kb + 4 * (lane >> 4);
    const float* w = flat + src + r;
    *reinterpret_cast<f32x4*>(packedT + idx) = f32x4{w[k * Rt], w[(k + 1) * Rt], w[(k + 2) * Rt], w[(k + 3) * Rt]};
}

// flat -> the split copies of the kSplitParam weights (policy_layout.hpp): one thread per lane of a
// (16-row tile, 32-k block), two f16x8 stores (w1 = f16(w), w2 = f16((w - w1) 2^11), round to nearest).
__global__ __launch_bounds__(256) void k_policy_split(const float* __restrict__ flat, float* __restrict__ packed) {
    const int i = blockIdx.x * 256 + tid_x();
    if (i < kRangeFloats) packed[kRangeOff + i] = 0.f;  // the range table, ahead of k_policy_range's maxima
    int si = 0, base = 0;
    while (si < kNumSplit && i >= base + kSizes[kSplitParam[si]] / 8) base += kSizes[kSplitParam[si++]] / 8;
    if (si >= kNumSplit) return;
    const int q = kSplitParam[si], K = kTileK[q], u = i - base;  // u = (t * K/32 + kb) * 64 + lane
    const int l = u & 63, blk = u >> 6, kb = blk % (K / 32), t = blk / (K / 32);
    const float* src = flat + kOffs.o[q] + (size_t)(16 * t + (l & 15)) * K + 32 * kb + 8 * (l >> 4);
    const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
    f16x8 w1, w2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float w = j < 4 ? a[j] : b[j - 4];
        w1[j] = (_Float16)w;
        w2[j] = f16_lo(w, w1[j]);
    }
    f16x8* dst = reinterpret_cast<f16x8*>(packed + kSplitOffs.o[si]) + (size_t)blk * 128 + l;
    dst[0] = w1;
    dst[64] = w2;
}

// The range table (policy_layout.hpp) of the flat parameters: kRangeSlices blocks per parameter,
// each an atomic max of its slice's max |param| on the float bits into the parameter's slot (zeroed
// by k_policy_split; non-negative floats order like their bits). One block per parameter looped
// over up to 49 k floats: 28 us per pack.
constexpr int kRangeSlices = 8;
__global__ __launch_bounds__(256) void k_policy_range(const float* __restrict__ flat, float* __restrict__ packed) {
    __shared__ float red[4];
    const int q = blockIdx.x / kRangeSlices, sl = blockIdx.x % kRangeSlices;
    const int n = kSizes[q], per = (n + kRangeSlices - 1) / kRangeSlices, i0 = sl * per, i1 = min(n, i0 + per);
    float m = 0.f;
    for (int i = i0 + tid_x(); i < i1; i += 256) m = fmaxf(m, fabsf(flat[kOffs.o[q] + i]));
    m = wave_max(m);
    if (lane_id() == 0) red[tid_x() >> 6] = m;
    __syncthreads();
    if (tid_x() == 0)
        atomicMax(reinterpret_cast<unsigned*>(packed + kRangeOff + kRgMax + q),
                  __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

int policy_split(const float* flat, float* packed, hipStream_t st) {
    constexpr int n = (kRangeOff - kOffs.o[kNumParams]) / 8;
    hipLaunchKernelGGL(k_policy_split, dim3((n + 255) / 256), dim3(256), 0, st, flat, packed);
    if (const int rc = check_launch("k_policy_split")) return rc;
    hipLaunchKernelGGL(k_policy_range, dim3(kNumParams * kRangeSlices), dim3(256), 0, st, flat, packed);
    return check_launch("k_policy_range");
}

// flat -> the split copies of the three layers' transposed weights (packedT + kTSplit): one thread
// per lane of a (16-row tile, 32-k block) of W^T, W^T[r][k] = W[k][r] gathered from the flat rows.
__global__ __launch_bounds__(256) void k_policyT_split(const float* __restrict__ flat, float* __restrict__ packedT) {
    const int i = blockIdx.x * 256 + tid_x();  // lane index over all 3 x kLayerT / 8 (tile, block, lane)
    if (i >= kHeadT / 8) return;
    const int li = i / (kLayerT / 8), loc = i - li * (kLayerT / 8);
    const int trunk = li == 0 ? kActorTrunk : kCriticTrunk, layer = li == 2 ? 1 : 0;
    int which, base, Rt, Kt;  // W^T is [Rt][Kt]; W flat [Kt][Rt]
    if (loc < kTWo / 8) { which = INW; base = kTWin; Rt = D; Kt = 3 * D; }
    else if (loc < kTW1 / 8) { which = OUTW; base = kTWo; Rt = D; Kt = D; }
    else if (loc < kTW2 / 8) { which = L1W; base = kTW1; Rt = D; Kt = FF; }
    else { which = L2W; base = kTW2; Rt = FF; Kt = D; }
    const int u = loc - base / 8, l = u & 63, blk = u >> 6, kb = blk % (Kt / 32), rt = blk / (Kt / 32);
    const int r = 16 * rt + (l & 15), k0 = 32 * kb + 8 * (l >> 4);
    const float* w = flat + kOffs.o[layer_param(trunk, layer, which)] + r;
    f16x8 w1, w2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = w[(size_t)(k0 + j) * Rt];
        w1[j] = (_Float16)v;
        w2[j] = f16_lo(v, w1[j]);
    }
    f16x8* dst = reinterpret_cast<f16x8*>(packedT + kTSplit + li * kLayerT + base) + (size_t)blk * 128 + l;
    dst[0] = w1;
    dst[64] = w2;
}

int policy_pack_train(const float* flat, float* packed, float* packedT, hipStream_t st) {
    const int items = kOffs.o[kNumParams] / 4 + kPackedTFloats / 4;
    hipLaunchKernelGGL(k_policy_pack, dim3((items + 255) / 256), dim3(256), 0, st, flat, packed, packedT);
    if (const int rc = check_launch("k_policy_pack")) return rc;
    hipLaunchKernelGGL(k_policyT_split, dim3((kHeadT / 8 + 255) / 256), dim3(256), 0, st, flat, packedT);
    if (const int rc = check_launch("k_policyT_split")) return rc;
    return policy_split(flat, packed, st);
}
}  // namespace pol
}  // namespace uavhip

extern "C" int uavhip_policy_pack(const float* flat, float* packed, uavhip_stream_t stream) {
    if (!flat || !packed) {
        set_error("uavhip_policy_pack: NULL pointer");
        return UAVHIP_EINVAL;
    }
    const int n = pol::kOffs.o[pol::kNumParams] / 4;
    hipLaunchKernelGGL(pol::k_policy_pack, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, flat, packed,
                       nullptr);
    if (const int rc = check_launch("k_policy_pack")) return rc;
    return pol::policy_split(flat, packed, (hipStream_t)stream);
}

extern "C" int32_t uavhip_policy_layout(int32_t* offsets, int32_t max_offsets) {
    if (offsets)
        for (int i = 0; i < pol::kNumParams && i < max_offsets; ++i) offsets[i] = pol::kOffs.o[i];
    return pol::kOffs.o[pol::kNumParams];
}

extern "C" int32_t uavhip_policy_split_layout(int32_t* params, int32_t* offsets, int32_t max_entries) {
    for (int i = 0; i < pol::kNumSplit && i < max_entries; ++i) {
        if (params) params[i] = pol::kSplitParam[i];
        if (offsets) offsets[i] = pol::kSplitOffs.o[i];
    }
    return pol::kPackedFloats;
}

extern "C" int32_t uavhip_policy_range_table(const float* max_abs, float* table) {
    if (!max_abs || !table) return pol::kRangeFloats;
    float t[pol::kRangeFloats] = {};
    for (int q = 0; q < pol::kNumParams; ++q) t[pol::kRgMax + q] = max_abs[q];
    pol::range_derive(t);
    for (int k = 0; k < pol::kRangeFloats; ++k) table[k] = t[k];
    return pol::kRangeFloats;
}

extern "C" int32_t uavhip_policy_tiling(int32_t* kcols, int32_t max_params) {
    if (kcols)
        for (int i = 0; i < pol::kNumParams && i < max_params; ++i) kcols[i] = pol::kTileK[i];
    return pol::kNumParams;
}

#ifdef UAVHIP_POLICY_TRACE
extern "C" int uavhip_policy_trace(unsigned long long* out, int n) {
    return copy_trace(pol::g_ptrace, 256 * 2 * pol::kTraceSlots, out, n);
}
extern "C" int uavhip_policy_btrace(unsigned long long* out, int n) {  // k_policy_backward stamps
    return copy_trace(pol::g_btrace, 256 * 2 * pol::kTraceSlots, out, n);
}
#endif

static int check_policy(const char* fn, const uavhip_policy* policy, const float* states, int32_t B) {
    if (!policy || !policy->weights || !states || B <= 0) {
        set_error("%s: NULL policy/weights/states or B=%d", fn, B);
        return UAVHIP_EINVAL;
    }
    if (policy->n_floats != pol::kPackedFloats || policy->d_model != pol::D || policy->n_heads != pol::NH ||
        policy->d_ff != pol::FF || policy->d_head_hidden != pol::HID || policy->actor_layers != 1 ||
        policy->critic_layers != 2) {
        set_error("%s: unsupported architecture / packed size %d (expected %d)", fn, policy->n_floats,
                  pol::kPackedFloats);
        return UAVHIP_EINVAL;
    }
    return UAVHIP_OK;
}

extern "C" int uavhip_policy_forward(const uavhip_policy* policy, const float* states, int32_t B,
                                     const int8_t* actions_in, uint64_t seed, uint64_t offset,
                                     const uint64_t* offset_dev, int8_t* action_out, float* logp, float* value,
                                     float* entropy, float* logits, uavhip_stream_t stream) {
    if (const int rc = check_policy("uavhip_policy_forward", policy, states, B)) return rc;
    const int grid = (B + pol::SPW - 1) / pol::SPW;
    hipLaunchKernelGGL(pol::k_policy_forward<false>, dim3(grid), dim3(pol::NTHR), 0, (hipStream_t)stream,
                       policy->weights, states, (int)B, actions_in, seed, offset, offset_dev, action_out, logp, value,
                       entropy, logits, pol::TrainIO{}, pol::RowIO{}, uavhip_env{}, pol::EnvOut{});
    return check_launch("k_policy_forward");
}

extern "C" int64_t uavhip_policy_rowproj_floats(int32_t B) {
    return B > 0 ? pol::kPposFloats + (int64_t)pol::S * B * pol::kRowFloats : -1;
}

// With `fill`: the ring rows of positions 0-3 of the B windows at `states` and the Win pos_s table
// (k_policy_rows_fill), ahead of a rows forward at rio.g.
static int ring_fill(const uavhip_policy* policy, const float* states, const pol::RowIO& rio, int32_t fill,
                     uavhip_stream_t stream) {
    if (!fill) return UAVHIP_OK;
    const int grid = (rio.B + pol::SPW - 1) / pol::SPW;
    hipLaunchKernelGGL(pol::k_policy_rows_fill, dim3(grid > pol::kPposParts ? grid : pol::kPposParts), dim3(pol::NTHR), 0,
                       (hipStream_t)stream, policy->weights, states, rio);
    return check_launch("k_policy_rows_fill");
}
// The ring of a rows forward over B windows, for entry point `fn` (`count`: its name for B in the message,
// "B" or "E"): the rowproj / step / 32-bit-offset check, the RowIO and the optional fill. `also_ok`: what
// the entry point requires besides, which `also` names in the message, after "NULL rowproj".
static int ring_setup(const char* fn, const char* count, const uavhip_policy* policy, const float* states, int32_t B,
                      float* rowproj, int32_t step, int32_t fill, uavhip_stream_t stream, pol::RowIO* rio,
                      const char* also = "", bool also_ok = true) {
    if (!rowproj || !also_ok || step < 0 || (int64_t)B * pol::S * pol::kRowFloats >= (int64_t)1 << 31) {
        set_error("%s: NULL rowproj%s, step=%d < 0 or %s=%d above the ring's 32-bit offsets", fn, also, step, count, B);
        return UAVHIP_EINVAL;
    }
    *rio = pol::RowIO{rowproj, (int)B, (int)step};
    return ring_fill(policy, states, *rio, fill, stream);
}

extern "C" int uavhip_policy_forward_rows(const uavhip_policy* policy, const float* states, int32_t B,
                                          float* rowproj, int32_t step, int32_t fill, const int8_t* actions_in,
                                          uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                                          int8_t* action_out, float* logp, float* value, float* entropy,
                                          float* logits, uavhip_stream_t stream) {
    if (const int rc = check_policy("uavhip_policy_forward_rows", policy, states, B)) return rc;
    pol::RowIO rio;
    if (const int rc = ring_setup("uavhip_policy_forward_rows", "B", policy, states, B, rowproj, step, fill, stream, &rio))
        return rc;
    const int grid = (B + pol::SPW - 1) / pol::SPW;
    hipLaunchKernelGGL((pol::k_policy_forward<false, true>), dim3(grid), dim3(pol::NTHR), 0, (hipStream_t)stream,
                       policy->weights, states, (int)B, actions_in, seed, offset, offset_dev, action_out, logp, value,
                       entropy, logits, pol::TrainIO{}, rio, uavhip_env{}, pol::EnvOut{});
    return check_launch("k_policy_forward_rows");
}

// Value-only ring forward (the rollout's bootstrap V(s_T)): the critic trunk and head of
// uavhip_policy_forward_rows, bitwise its value output; the actor's ring row is not written.
extern "C" int uavhip_policy_value_rows(const uavhip_policy* policy, const float* states, int32_t B, float* rowproj,
                                        int32_t step, int32_t fill, float* value, uavhip_stream_t stream) {
    if (const int rc = check_policy("uavhip_policy_value_rows", policy, states, B)) return rc;
    pol::RowIO rio;
    if (const int rc = ring_setup("uavhip_policy_value_rows", "B", policy, states, B, rowproj, step, fill, stream, &rio,
                                  " / value", value != nullptr))
        return rc;
    const int grid = (B + pol::SPW - 1) / pol::SPW;
    hipLaunchKernelGGL((pol::k_policy_forward<false, true, 0, true>), dim3(grid), dim3(pol::NTHR), 0, (hipStream_t)stream,
                       policy->weights, states, (int)B, nullptr, 0ull, 0ull, nullptr, nullptr, nullptr, value, nullptr,
                       nullptr, pol::TrainIO{}, rio, uavhip_env{}, pol::EnvOut{});
    return check_launch("k_policy_value_rows");
}

// What the four fused step entry points share ahead of their launch, for entry point `fn`: the env
// (B = env->E windows), the policy, one env per wave (N, M <= 64), f32 observations where `f32_only`,
// the entry point's own arguments (`args_ok`; `need`, a format and its values, names them in the
// message), the ring on the windows at `states` (slot step & 1 of two where `two_slots`) and the floats
// of B windows.
struct StepSetup {
    int32_t B;
    long long stride;
    pol::RowIO rio;
};
static int step_setup(StepSetup* su, const char* fn, const uavhip_policy* policy, const uavhip_env* env,
                      const float* states, bool two_slots, float* rowproj, int32_t step, int32_t fill,
                      uavhip_stream_t stream, bool f32_only, bool args_ok, const char* need, ...) {
    if (const int rc = validate_env(env, true)) return rc;
    su->B = env->E;
    su->stride = (long long)su->B * pol::S * pol::IN;
    if (const int rc = check_policy(fn, policy, states, su->B)) return rc;
    if (env->N > 64 || env->M > 64 || (f32_only && require_f32_obs(fn, env)) || !args_ok) {
        char rest[160];  // (require_f32_obs' own message is replaced by the entry point's, which names every condition)
        va_list ap;
        va_start(ap, need);
        vsnprintf(rest, sizeof rest, need, ap);
        va_end(ap);
        set_error("%s: N=%d, M=%d must be <= 64%s%s", fn, env->N, env->M, f32_only ? ", observations f32" : "", rest);
        return UAVHIP_EINVAL;
    }
    return ring_setup(fn, "E", policy, states + (two_slots ? (step & 1) * su->stride : 0), su->B, rowproj, step, fill,
                      stream, &su->rio);
}

// Fused rollout step: uavhip_policy_forward_rows (sampling) + uavhip_env_step (T = 1) of env e
// on window b = e, one launch. N, M <= 64 (one env per wave); B = env->E.
extern "C" int uavhip_rollout_step(const uavhip_policy* policy, const uavhip_env* env, const float* states,
                                   float* rowproj, int32_t step, int32_t fill, uint64_t seed, uint64_t offset,
                                   const uint64_t* offset_dev, int8_t* action_out, float* logp, float* value,
                                   int32_t auto_reset, float* obs_out, double* reward, uint8_t* done, double* info,
                                   uavhip_stream_t stream) {
    StepSetup su;
    if (const int rc = step_setup(&su, "uavhip_rollout_step", policy, env, states, false, rowproj, step, fill, stream, false,
                                  action_out && obs_out && reward && done, " and action/obs/reward/done non-NULL"))
        return rc;
    const int grid = (su.B + pol::SPW - 1) / pol::SPW;
    hipLaunchKernelGGL((pol::k_policy_forward<false, true, pol::kEnvBoth>), dim3(grid), dim3(pol::NTHR), 0, (hipStream_t)stream,
                       policy->weights, states, (int)su.B, nullptr, seed, offset, offset_dev, action_out, logp, value,
                       nullptr, nullptr, pol::TrainIO{}, su.rio, *env,
                       pol::EnvOut{(int)auto_reset, obs_out, reward, done, info});
    return check_launch("k_rollout_step");
}

extern "C" int uavhip_rollout_steps(const uavhip_policy* policy, const uavhip_env* env, float* obs, float* rowproj,
                                    int32_t step, int32_t n, int32_t fill, uint64_t seed, uint64_t offset,
                                    uint64_t offset_stride, const uint64_t* offset_dev, int8_t* actions, float* logp,
                                    float* value, int32_t auto_reset, double* reward, uint8_t* done, double* info,
                                    uavhip_stream_t stream) {
    StepSetup su;
    if (const int rc = step_setup(&su, "uavhip_rollout_steps", policy, env, obs, false, rowproj, step, fill, stream, true,
                                  actions && logp && value && reward && done && n > 0,
                                  ", n=%d > 0 and actions/logp/value/reward/done non-NULL", n))
        return rc;
    return pol::launch_rollout_steps(
        pol::StepsArgs{policy->weights, obs, (int)su.B, seed, offset, offset_dev, actions, logp, value, su.rio, *env,
                       pol::EnvOut{(int)auto_reset, obs + su.stride, reward, done, info},
                       pol::StepSeq{(int)n, su.stride, offset_stride}},
        (hipStream_t)stream);
}

// uavhip_rollout_steps without the critic (k_rollout_actor_steps); uavhip_value_steps supplies the values.
extern "C" int uavhip_rollout_actor_steps(const uavhip_policy* policy, const uavhip_env* env, float* obs,
                                          float* rowproj, int32_t step, int32_t n, int32_t fill, uint64_t seed,
                                          uint64_t offset, uint64_t offset_stride, const uint64_t* offset_dev,
                                          int8_t* actions, float* logp, int32_t auto_reset, double* reward,
                                          uint8_t* done, double* info, uavhip_stream_t stream) {
    StepSetup su;
    if (const int rc = step_setup(&su, "uavhip_rollout_actor_steps", policy, env, obs, false, rowproj, step, fill, stream,
                                  true, actions && logp && reward && done && n > 0,
                                  ", n=%d > 0 and actions/logp/reward/done non-NULL", n))
        return rc;
    return pol::launch_rollout_actor_steps(
        pol::StepsArgs{policy->weights, obs, (int)su.B, seed, offset, offset_dev, actions, logp, nullptr, su.rio, *env,
                       pol::EnvOut{(int)auto_reset, obs + su.stride, reward, done, info},
                       pol::StepSeq{(int)n, su.stride, offset_stride}},
        (hipStream_t)stream);
}

// The values of the recorded windows obs[0 .. n - 1] (and of obs[n] when last_values is given) on the
// critic's ring rows, one launch (k_value_steps).
extern "C" int64_t uavhip_value_steps_stash_floats(int32_t B) {
    return B > 0 ? (int64_t)((B + pol::SPW - 1) / pol::SPW) * pol::kVG * 2 * pol::SPW * (pol::D + 8) : -1;
}
extern "C" int uavhip_value_steps(const uavhip_policy* policy, const float* obs, int32_t B, int32_t n, float* rowproj,
                                  int32_t step, int32_t fill, float* values, float* last_values, float* stash,
                                  uavhip_stream_t stream) {
    if (const int rc = check_policy("uavhip_value_steps", policy, obs, B)) return rc;
    char also[64];
    snprintf(also, sizeof also, " / values / stash, n=%d <= 0", n);
    pol::RowIO rio;
    if (const int rc = ring_setup("uavhip_value_steps", "B", policy, obs, B, rowproj, step, fill, stream, &rio, also,
                                  values && stash && n > 0))
        return rc;
    return pol::launch_value_steps(pol::ValueArgs{policy->weights, obs, (int)B, (int)n, (long long)B * pol::S * pol::IN,
                                                  rio, values, last_values, stash},
                                   (hipStream_t)stream);
}

// Inference: up to n_max actor-only steps of every env in one launch (k_decode_steps).
extern "C" int uavhip_decode_steps(const uavhip_policy* policy, const uavhip_env* env, float* obs2, float* rowproj,
                                   int32_t step, int32_t n_max, int32_t fill, int32_t greedy_stride, uint64_t seed,
                                   uint64_t offset, uint64_t offset_stride, const uint64_t* offset_dev,
                                   int8_t* actions, int32_t* steps, uint8_t* finished, double* ep_return,
                                   uavhip_stream_t stream) {
    StepSetup su;
    if (const int rc = step_setup(&su, "uavhip_decode_steps", policy, env, obs2, true, rowproj, step, fill, stream, true,
                                  n_max > 0 && greedy_stride >= 0 && steps && finished,
                                  ", n_max=%d > 0, greedy_stride=%d >= 0 and steps/finished non-NULL", n_max, greedy_stride))
        return rc;
    return pol::launch_decode_steps(pol::DecodeArgs{policy->weights, obs2, (int)su.B, seed, offset, offset_dev, su.rio,
                                                    *env, (int)n_max, (int)greedy_stride, su.stride, offset_stride,
                                                    actions, steps, finished, ep_return},
                                    (hipStream_t)stream);
}
