// policy_encoder.hpp -- the encoder of one trunk on a workgroup's 80 tokens: the fused LayerNorm epilogue,
// attention, the embedding, layer_tail and the encoder_layer* variants, and the window-row ring path
// (RowIO ... rows_prologue). Included by policy.hip and rollout_steps.hip (through policy_block.hpp).
#pragma once
#include "policy_core.hpp"

namespace uavhip {
namespace pol {

// Fused GEMM epilogue + post-LN (nn.TransformerEncoderLayer norm1 / norm2, eps 1e-5):
//   h[tok][f] = LN(h[tok] + acc + bias)[f] * w[f] + b[f]
// for this wave's 16 output features f = [16 wv, 16 wv + 16) of CT column tiles from ytok0. The
// token statistics combine per-wave (mean, M2) pairs over 16 features each (Chan et al.), so one
// barrier suffices and the variance is two-pass accurate. Ends WITHOUT a barrier after writing h.
// Training-mode outputs of a LayerNorm: normalised rows, output rows, 1/std per row, in the
// workspace layout (compact [b] rows for the pruned tail, [b * 5 + s] rows otherwise).
struct LnOut {
    float *x, *h, *rs;
    int b0, compact;
    bool nt = true;  // non-temporal stores (act_st): not in the position-split kernels
};
__device__ __forceinline__ int trow(int tok, int b0) { return (b0 + (tok & (SPW - 1))) * S + tok / SPW; }
__device__ __forceinline__ int orow(int tok, int b0, bool compact) {
    return compact ? b0 + (tok & (SPW - 1)) : trow(tok, b0);
}

// The epilogue's per-feature operands: the GEMM bias, loaded by the caller BEFORE the GEMM (the
// epilogue's first instruction needs it, so a load issued after the GEMM would expose a whole L2
// round trip), and the LN weight and bias, loaded right after the GEMM -- ahead of its next
// prefetches and the barrier, whose latency then covers them.
struct LnPar {
    f32x4 bb, ww, lb;
};
__device__ __forceinline__ f32x4 ln_bias(TID_F const float* __restrict__ bias) {
    return *reinterpret_cast<const f32x4*>(bias + 16 * (TIDX() >> 6) + 4 * (LANE() >> 4));
}
__device__ __forceinline__ LnPar ln_load(TID_F const f32x4 bb, const float* __restrict__ w, const float* __restrict__ b) {
    const int f0 = 16 * (TIDX() >> 6) + 4 * (LANE() >> 4);
    return LnPar{bb, *reinterpret_cast<const f32x4*>(w + f0), *reinterpret_cast<const f32x4*>(b + f0)};
}
// PLANES: the output goes to sm.h as the two fp16 planes of the split products (the next GEMM's
// operand; the caller keeps the fp32 output from `outv`); resid: the residual from registers (the
// lane's own elements, as `outv` returned them) instead of sm.h.
// ROW4 (with PLANES): the fp32 output of position 4 (tokens 64-79) also goes to sm.ctx rows 0-15 (the
// next, pruned layer's residual and query rows). psc: the planes' scale (the operand's 2^-s).
// T0 / T1 / T2 (trace builds, >= 0): phase stamps when the GEMM accumulators are consumed, when the
// partial statistics are written, after the barrier
template <int CT, bool TR = false, bool PLANES = false, bool ROW4 = false, int T0 = -1, int T1 = -1, int T2 = -1>
__device__ __forceinline__ void residual_layernorm(TID_F Smem& sm, const f32x4 (&acc)[CT], const LnPar& lp, int ytok0,
                                                   const LnOut& lo = LnOut{}, f32x4* outv = nullptr,
                                                   const f32x4* resid = nullptr, float psc = 1.f) {
    const int l = LANE(), i16 = l & 15, g = l >> 4, wv = TIDX() >> 6;
    const int f0 = 16 * wv + 4 * g;
    const f32x4 bb = lp.bb;
    f32x4 v[CT];
#if defined(UAVHIP_POLICY_TRACE)
    if constexpr (T0 >= 0) {
        float dep = 0.f;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) dep += acc[ct].x;
        asm volatile("" ::"v"(dep));
        __builtin_amdgcn_sched_barrier(0);
        PTR(T0);
    }
#endif
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int tok = ytok0 + 16 * ct + i16;
        v[ct] = acc[ct] + bb + (resid ? resid[ct] : *reinterpret_cast<const f32x4*>(sm.h + tok * LDH + f0));
        float s = (v[ct].x + v[ct].y) + (v[ct].z + v[ct].w);
        s = add_xor32(add_xor16(s));
        const float m = s * (1.0f / 16);
        const f32x4 d = v[ct] - m;
        float q = (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
        q = add_xor32(add_xor16(q));
        if (g == 0) sm.red[wv * TOK + tok] = make_float2(m, q);
    }
#if defined(UAVHIP_POLICY_TRACE)
    if constexpr (T1 >= 0) {
        __builtin_amdgcn_sched_barrier(0);
        PTR(T1);
    }
#endif
    __syncthreads();
#if defined(UAVHIP_POLICY_TRACE)
    if constexpr (T2 >= 0) PTR(T2);
#endif
    const f32x4 ww = lp.ww, lb = lp.lb;
    // (mean, 1/std) of token tok from the 8 per-wave partials
    auto stats = [&](int tok, float& mean, float& rs) {
        float2 pr[NW];
        float ms = 0.f;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            pr[k] = sm.red[k * TOK + tok];
            ms += pr[k].x;
        }
        mean = ms * (1.0f / NW);
        float m2 = 0.f;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const float dm = pr[k].x - mean;
            m2 += pr[k].y + 16.0f * dm * dm;
        }
        rs = ln_rstd(m2 * (1.0f / D) + 1e-5f);
    };
    static_assert(CT == 1 || CT == S, "pruned tile or all five");
    // all five tiles: lane (i16, g) combines the partials of tile g's token, the last tile's in a
    // second round; the other rows of the wave fetch theirs with ds_bpermute (instead of every row
    // of the wave redoing every token's combine)
    float mA, rA, mB, rB;
    if constexpr (CT == 1) stats(ytok0 + i16, mA, rA);
    else {
        stats(ytok0 + 16 * g + i16, mA, rA);
        stats(ytok0 + 16 * (S - 1) + i16, mB, rB);
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int tok = ytok0 + 16 * ct + i16;
        float mean = mA, rs = rA;
        if (CT > 1 && ct < S - 1) {
            mean = __shfl(mA, 16 * ct + i16);
            rs = __shfl(rA, 16 * ct + i16);
        } else if (CT > 1) {
            mean = mB;
            rs = rB;
        }
        const f32x4 xh = (v[ct] - mean) * rs;
        const f32x4 out = xh * ww + lb;
        if constexpr (PLANES) hsplit_store(reinterpret_cast<_Float16*>(sm.h), psw(tok, f0), out * psc);
        else *reinterpret_cast<f32x4*>(sm.h + tok * LDH + f0) = out;
        if constexpr (ROW4) {
            if (ct == CT - 1) *reinterpret_cast<f32x4*>(sm.ctx + (tok - (S - 1) * SPW) * LDH + f0) = out;
        }
        if (outv) outv[ct] = out;
        if (TR) {
            const size_t r = (size_t)orow(tok, lo.b0, lo.compact);
            act_st(lo.x + r * D + f0, xh, lo.nt);
            if (lo.h) act_st(lo.h + r * D + f0, out, lo.nt);  // nullptr: formed by k_wgrad
            if (wv == 0 && g == 0) lo.rs[r] = rs;
        }
    }
}

// Full-layer attention for heads [4c, 4c+4): one (sample, head, query group) task per 4 lanes,
// each lane owning 4 of the 16 head dims; the task loads the 5 keys / values once for all its
// queries (group 0: positions 0-2 on waves 0-3, group 1: positions 3-4 on waves 4-7).
// attention_full_core leaves the outputs in registers (o[qi] for query position qs0 + qi, qi < nq);
// attention_full_store writes them to sm.ctx as the split products' fp16 planes.
__device__ __forceinline__ void attention_full_core(TID_F Smem& sm, int c, f32x4 (&o)[3]) {
    const int q4 = TIDX() & 3, task = TIDX() >> 2;
    const int hh = task & 3, p = (task >> 2) & 15, grp = task >> 6;
    const int d0 = hh * HD + 4 * q4;
    f32x4 k[S], v[S];
    bool msk[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
        k[j] = *reinterpret_cast<const f32x4*>(sm.big + (j * SPW + p) * LDB + 64 + d0);
        v[j] = *reinterpret_cast<const f32x4*>(sm.big + (j * SPW + p) * LDB + 128 + d0);
        msk[j] = sm.mask[p * S + j] != 0;
    }
    const int qs0 = grp ? 3 : 0, nq = grp ? 2 : 3;
#pragma unroll
    for (int qi = 0; qi < 3; ++qi) {
        o[qi] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (qi < nq) {
            const int ti = (qs0 + qi) * SPW + p;
            const f32x4 q = *reinterpret_cast<const f32x4*>(sm.big + ti * LDB + d0) * kAttQ;
            float sc[S];
            float mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                float part = att_dot(q, k[j]);
                part = add_xor2(add_xor1(part));
                sc[j] = msk[j] ? -INFINITY : part;
                mx = j ? fmaxf(mx, sc[j]) : sc[j];
            }
            float den = 0.f;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                sc[j] = __expf(sc[j] - mx);
                den = j ? den + sc[j] : sc[j];
            }
            const float inv = att_recip(den);
            att_mix(o[qi], sc, inv, v);
        }
    }
}
// sc: the planes' scale, of this thread's sample p (att_sc)
__device__ __forceinline__ void attention_full_store(TID_F Smem& sm, int c, const f32x4 (&o)[3], float sc) {
    const int q4 = TIDX() & 3, task = TIDX() >> 2;
    const int hh = task & 3, p = (task >> 2) & 15, grp = task >> 6;
    const int d0 = hh * HD + 4 * q4, qs0 = grp ? 3 : 0, nq = grp ? 2 : 3;
#pragma unroll
    for (int qi = 0; qi < 3; ++qi) {
        if (qi < nq) {
            const int ti = (qs0 + qi) * SPW + p;
            hsplit_store(reinterpret_cast<_Float16*>(sm.ctx), psw(ti, 4 * c * HD + d0), o[qi] * sc);
        }
    }
}
// The output goes to sm.ctx as the two fp16 planes of the split products (the out-projection's
// operand), scaled for layer `layer` of trunk `trunk`.
// (no defaults: every call site names the operand whose scale the planes carry -- ADVICE r05)
template <int trunk, int layer>
__device__ void attention_full(TID_F Smem& sm, int c, const float* __restrict__ P = nullptr) {
    f32x4 o[3];
    attention_full_core(TID_C sm, c, o);
    attention_full_store(TID_C sm, c, o, att_sc<trunk, layer>(sm, (int)((TIDX() >> 4) & 15)).sc);
}

// Scaled-dot-product attention for heads [4c, 4c+4) of the query positions [qs0, qs0 + nqs) over
// the keys/values of all 5 positions; reads sm.big (Q|K|V of the chunk), writes sm.ctx.
// One (query, head) task per 4 consecutive lanes, each lane owning 4 of the 16 head dims
// (dot products reduced over the quad with two xor-shuffles). _core: one query position (nqs = 1):
// threads < 256 own one task each, its output in `o`.
// Two lane mappings compute this arithmetic. Here, the LDS mapping: the quad is lane bits 0-1 (lane q4
// owns dims 4 q4 .. 4 q4 + 3), reduced with add_xor1 then add_xor2. In attention_head, the MFMA tile
// mapping: the quad is lane bits 4-5 (lane (p, g) owns dims 4g .. 4g + 3), reduced with add_xor16 then
// add_xor32. Either tree adds the partner across the quad's low bit first, then across its high bit:
// (d0 + d1) + (d2 + d3) in every lane, each sum of the same two values (IEEE addition commutes), so the
// scores -- and everything after them, which is per lane -- are bitwise equal.
__device__ __forceinline__ void attention_task(TID_F Smem& sm, int task, int qs0, f32x4& o, int& ti, int& d0) {
    const int q4 = TIDX() & 3;
    const int hh = task & 3, rest = task >> 2, p = rest & 15, si = qs0 + (rest >> 4);
    ti = si * SPW + p;
    d0 = hh * HD + 4 * q4;
    const f32x4 q = *reinterpret_cast<const f32x4*>(sm.big + ti * LDB + d0) * kAttQ;
    float sc[S];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const f32x4 k = *reinterpret_cast<const f32x4*>(sm.big + (j * SPW + p) * LDB + 64 + d0);
        float part = att_dot(q, k);
        part = add_xor2(add_xor1(part));
        sc[j] = sm.mask[p * S + j] ? -INFINITY : part;
        mx = j ? fmaxf(mx, sc[j]) : sc[j];
    }
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < S; ++j) {
        sc[j] = __expf(sc[j] - mx);
        den = j ? den + sc[j] : sc[j];
    }
    const float inv = att_recip(den);
    f32x4 v[S];
#pragma unroll
    for (int j = 0; j < S; ++j) v[j] = *reinterpret_cast<const f32x4*>(sm.big + (j * SPW + p) * LDB + 128 + d0);
    o = f32x4{0.f, 0.f, 0.f, 0.f};
    att_mix(o, sc, inv, v);
}
__device__ __forceinline__ void attention_out(TID_F Smem& sm, int c, int ti, int d0, const f32x4 o, float sc) {
    hsplit_store(reinterpret_cast<_Float16*>(sm.ctx), psw(ti, 4 * c * HD + d0), o * sc);
}
// attention_task for ONE head with the operands already in registers, in the lane mapping of a 16-row
// MFMA output tile: lane (p = lane & 15, g = lane >> 4) holds dims 4g .. 4g + 3 of sample p's query, keys
// and values (k[j], v[j]: position j), the head being the wave's. The quad of attention_task (lane bits
// 0-1, add_xor1 then add_xor2) sits on lane bits 4-5 here (add_xor16 then add_xor32): both trees form
// (d0 + d1) + (d2 + d3) of the four lanes' partial dots, and the two operands of every sum are the same
// pair of values, so each score is bitwise attention_task's. Everything else is its arithmetic, lane by
// lane. Returns the lane's four output dims (unscaled).
// attention_weights: the first half -- e[j] = exp(score_j - max) and 1 / sum(e), the same in the four lanes
// of a quad; att_mix with the values is the second.
__device__ __forceinline__ float attention_weights(TID_F const Smem& sm, const f32x4 q_, const f32x4 (&k)[S],
                                                   float (&sc)[S]) {
    const int p = LANE() & 15;
    const f32x4 q = q_ * kAttQ;
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < S; ++j) {
        float part = att_dot(q, k[j]);
        part = add_xor32(add_xor16(part));
        sc[j] = sm.mask[p * S + j] ? -INFINITY : part;
        mx = j ? fmaxf(mx, sc[j]) : sc[j];
    }
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < S; ++j) {
        sc[j] = __expf(sc[j] - mx);
        den = j ? den + sc[j] : sc[j];
    }
    return att_recip(den);
}
__device__ __forceinline__ f32x4 attention_head(TID_F const Smem& sm, const f32x4 q_, const f32x4 (&k)[S],
                                                const f32x4 (&v)[S]) {
    float sc[S];
    const float inv = attention_weights(TID_C sm, q_, k, sc);
    f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
    att_mix(o, sc, inv, v);
    return o;
}
template <int trunk, int layer>
__device__ void attention_chunk(TID_F Smem& sm, int c, int qs0, int nqs, const float* __restrict__ P = nullptr) {
    const int ntask = nqs * SPW * 4;
    for (int task = TIDX() >> 2; task < ntask; task += NTHR / 4) {
        f32x4 o;
        int ti, d0;
        attention_task(TID_C sm, task, qs0, o, ti, d0);
        attention_out(TID_C sm, c, ti, d0, o, att_sc<trunk, layer>(sm, ti & 15).sc);
    }
}

// Embedding (transformer_net.py:57-59) on the MFMA, K = 14 padded to 16 with zeros:
// h[s*16+p][f] = relu(W_e x[p][s] + b_e)[f] + pos[s][f]; wave w computes features [16w, 16w+16).
// The global operands (weights, bias, position rows) are loaded up front (embed_load), so a caller
// can issue later loads behind them without the embedding waiting for those (in-order vmcnt).
struct EmbPre {
    f32x4 a, bb, pp[S];
};
template <int trunk>
__device__ __forceinline__ EmbPre embed_load(TID_F const float* __restrict__ P) {
    const float* We = P + kOffs.o[trunk + EMB_W];
    const float* be = P + kOffs.o[trunk + EMB_B];
    const float* pos = P + kOffs.o[trunk + POS];
    const int l = LANE(), i16 = l & 15, g = l >> 4, wv = TIDX() >> 6;
    const int f = 16 * wv + i16;
    EmbPre r;
    r.a.x = 4 * g + 0 < IN ? We[f * IN + 4 * g + 0] : 0.f;
    r.a.y = 4 * g + 1 < IN ? We[f * IN + 4 * g + 1] : 0.f;
    r.a.z = 4 * g + 2 < IN ? We[f * IN + 4 * g + 2] : 0.f;
    r.a.w = 4 * g + 3 < IN ? We[f * IN + 4 * g + 3] : 0.f;
    r.bb = *reinterpret_cast<const f32x4*>(be + 16 * wv + 4 * g);
#pragma unroll
    for (int ct = 0; ct < S; ++ct) r.pp[ct] = *reinterpret_cast<const f32x4*>(pos + ct * D + 16 * wv + 4 * g);
    return r;
}
// MODE kEmbH: h = e + pos for all 5 positions (sm.h). kEmbSplit: also e of position 4 (no pos)
// -> sm.ctx rows 64-79 (the window-row projection path's in_proj input). kEmbRows: only e of
// positions 0-3 -> sm.ctx (row projection fill). kEmbOne (the actor-only step, encoder_layer_rows
// ONEPASS): kEmbSplit, but the planes of e of position 4 go to sm.big rows 0-15 -- its attention writes
// sm.ctx rows 64-79 with no barrier after the new-row GEMM, whose operand must then live elsewhere.
enum { kEmbH = 0, kEmbSplit = 1, kEmbRows = 2, kEmbOne = 3 };
// PL (kEmbH): also the two fp16 planes of h into sm.ctx (the split layer-0 in_proj's operand,
// encoder_layer_split).
template <int trunk, bool TR = false, int MODE = kEmbH, bool PL = false>
__device__ void embed_apply(TID_F Smem& sm, const EmbPre& ep, float* e_out = nullptr, float* h_out = nullptr, int b0 = 0) {
    const int l = LANE(), i16 = l & 15, g = l >> 4, wv = TIDX() >> 6;
    constexpr int NT = MODE == kEmbRows ? S - 1 : S;
    // the ring forward's actor (its only layer is pruned to position 4): positions 0-3 come from the
    // ring rows and only position 4 is a residual, so only its embedding is formed
    constexpr int CT0 = (MODE == kEmbSplit || MODE == kEmbOne) && trunk == kActorTrunk ? S - 1 : 0;
    static_assert(MODE != kEmbOne || (trunk == kActorTrunk && split_slot(layer_param(trunk, 0, INW)) >= 0),
                  "the actor's one-pass step: a split new-row GEMM");
    f32x4 acc[NT];
#pragma unroll
    for (int ct = CT0; ct < NT; ++ct) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(sm.x + (ct * SPW + i16) * LDX + 4 * g);
        acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(ep.a[j], b[j], acc[ct], 0, 0, 0);
    }
#pragma unroll
    for (int ct = CT0; ct < NT; ++ct) {
        f32x4 e = acc[ct] + ep.bb;
        e.x = fmaxf(e.x, 0.f); e.y = fmaxf(e.y, 0.f); e.z = fmaxf(e.z, 0.f); e.w = fmaxf(e.w, 0.f);
        const int o = (ct * SPW + i16) * LDH + 16 * wv + 4 * g;
        constexpr bool ring_planes = split_slot(layer_param(trunk, 0, INW)) >= 0;  // the ring GEMM's operand
        // the planes of layer 0's input scaled per token (its window row's range)
        const float esc = (ring_planes || PL) ? es_factor<trunk, -1>(sm, ct * SPW + i16) : 1.f;
        if (MODE == kEmbOne && ct == S - 1)
            hsplit_store(reinterpret_cast<_Float16*>(sm.big), psw(i16, 16 * wv + 4 * g), e * esc);
        else if ((MODE == kEmbRows || (MODE == kEmbSplit && ct == S - 1)) && ring_planes)
            hsplit_store(reinterpret_cast<_Float16*>(sm.ctx), psw((ct * SPW + i16), 16 * wv + 4 * g), e * esc);
        else if (MODE == kEmbRows || (MODE == kEmbSplit && ct == S - 1)) *reinterpret_cast<f32x4*>(sm.ctx + o) = e;
        if (MODE == kEmbRows) continue;
        const f32x4 v = e + ep.pp[ct];
        *reinterpret_cast<f32x4*>(sm.h + o) = v;
        if constexpr (PL) hsplit_store(reinterpret_cast<_Float16*>(sm.ctx), psw((ct * SPW + i16), 16 * wv + 4 * g), v * esc);
        if (TR) {
            const size_t r = (size_t)trow(ct * SPW + i16, b0);
            act_st(e_out + r * D + 16 * wv + 4 * g, e);
            if (h_out) act_st(h_out + r * D + 16 * wv + 4 * g, v);
        }
    }
}
template <int trunk, bool TR = false>
__device__ void embed(TID_F Smem& sm, const float* __restrict__ P, float* e_out = nullptr, float* h_out = nullptr,
                      int b0 = 0) {
    embed_apply<trunk, TR>(TID_C sm, embed_load<trunk>(TID_C P), e_out, h_out, b0);
}

// K/V weight row of wave wv for chunk c: waves 0-3 K tiles, waves 4-7 V tiles
__device__ __forceinline__ int kv_row(int wv, int c) { return (1 + (wv >> 2)) * D + 64 * c + 16 * (wv & 3); }

// A caller's hook run inside layer_tail after the FFN2 GEMM, before the LN2 epilogue (training
// mode: the next phase's global loads issued ahead of LN2's activation stores -- the vector memory
// counter retires in order, so a load behind a store burst waits for the whole burst).
struct NoHook {
    __device__ void operator()() const {}
};
// Every layer's out-projection and FFN run as split products (policy_layout.hpp kSplitParam: every
// layer GEMM weight has a split copy). A layer whose in_proj does too takes K / V / Q from the fp16
// planes of its input, which the previous layer's LN2 then writes:
template <int trunk, int layer>
constexpr bool split_inproj() {  // layer >= 1: its input comes from a full layer's LN2 (layer 0's in_proj
                                 // split copy serves the window-row ring and the training forward)
    return layer >= 1 && layer < 2 && split_slot(layer_param(trunk, layer, INW)) >= 0;
}
// Weight blocks (of 32 k) a tail GEMM has in registers before its k-loop starts
constexpr int kTailDepth = 2;
// The caller's prefetch of a layer tail's first out-projection weight blocks (layer_tail's `po`)
using TailPre = HPre<kTailDepth>;
// (last, TR: unused, but they keep one instantiation per kind of caller. Invariant as layer_tail_fwd's:
// with the pruned and the batched critic tails sharing one, k_value_steps' code object holds the same
// instructions in another register numbering. Fold them away only together with a same-box benchmark of
// k_value_steps.)
template <int trunk, int layer, bool last, bool TR>
__device__ __forceinline__ TailPre tail_prefetch(TID_F const float* __restrict__ P) {
    const int wv = TIDX() >> 6;
    return hprefetch<kTailDepth>(TID_C P, split_slot(layer_param(trunk, layer, OUTW)), D, 16 * wv, 0);
}
// Whether a layer's in_proj runs as split products (encoder_layer_split): when the previous layer's
// LN2 wrote its input's planes, and for layer 0 of the training forward (the embedding's planes).
// Otherwise -- layer 0 of the inference forward without the window-row ring -- it runs on the f32
// MFMA (linear1). KvPre / kv_prefetch: the caller's prefetch of the layer's first K/V weight blocks.
template <int trunk, int layer, bool TR>
constexpr bool split_kv() {
    return split_inproj<trunk, layer>() || (TR && layer == 0);
}
template <int trunk, int layer, bool TR>
using KvPre = std::conditional_t<split_kv<trunk, layer, TR>(), HPre<2>, APre<2>>;
template <int trunk, int layer, bool TR>
__device__ __forceinline__ KvPre<trunk, layer, TR> kv_prefetch(TID_F const float* __restrict__ P) {
    const int wv = TIDX() >> 6;
    if constexpr (split_kv<trunk, layer, TR>())
        return hprefetch<2>(TID_C P, split_slot(layer_param(trunk, layer, INW)), D, kv_row(wv, 0), 0);
    else
        return prefetch<2>(TID_C P + kOffs.o[layer_param(trunk, layer, INW)], D, kv_row(wv, 0), 0);
}

// Training mode: the Q|K|V of chunk c of the tokens [qtok0, 80) (Q) / all (K, V) from sm.big to qkv
// rows, by waves 4-7 (less MFMA work than the K + Q waves sharing their SIMDs).
__device__ __forceinline__ void store_qkv_chunk(TID_F const Smem& sm, float* __restrict__ qkv, int c, int qtok0, int b0) {
    for (int i = (int)TIDX() - NTHR / 2; i < TOK * 48; i += NTHR / 2) {
        if (i < 0) break;
        const int tok = i / 48, r = i - tok * 48, part = r >> 4, q = r & 15;
        if (part == 0 && tok < qtok0) continue;
        act_st(qkv + (size_t)trow(tok, b0) * 3 * D + part * D + 64 * c + 4 * q,
               *reinterpret_cast<const f32x4*>(sm.big + tok * LDB + part * 64 + 4 * q));
    }
}
// Training mode: fp32 rows from the two planes of a split-product operand in LDS (the values the
// GEMM consumed: (x1 + 2^-11 x2) 2^s, inv(tok) = 2^s of the token's operand scale) -> workspace rows
// (stride ldo, column offset c0), tokens [t0, t1).
template <class Inv>
__device__ __forceinline__ void store_rows_planes(TID_F const _Float16* src, float* dst, int ldo, int c0, int ncols,
                                                  int t0, int b0, bool compact, int t1, Inv inv, bool nt = true) {
    const int n4 = ncols / 4, items = (t1 - t0) * n4;
    for (int i = TIDX(); i < items; i += NTHR) {
        const int tok = t0 + i / n4, q = i % n4;
        const f16x4 x1 = *reinterpret_cast<const f16x4*>(src + psw(tok, 4 * q));
        const f16x4 x2 = *reinterpret_cast<const f16x4*>(src + kPlane + psw(tok, 4 * q));
        const float s = inv(tok);
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ((float)x1[j] + (float)x2[j] * kLoScale) * s;
        act_st(dst + (size_t)orow(tok, b0, compact) * ldo + c0 + 4 * q, v, nt);
    }
}

// 2^s of a layer's in_proj operand at token tok: layer 0's input per token (its window row's range),
// a later layer's input = the previous layer's LN2 output (static)
template <int trunk, int layer>
__device__ __forceinline__ float in_inv(const Smem& sm, int tok) {
    if constexpr (layer == 0) return es_factor<trunk, 1>(sm, tok);
    else return op_sc<trunk, layer - 1, kOpLn2>(sm).inv;
}

// Out-projection + LN1 + FFN + LN2 of an encoder layer as split products, after the attention
// output's planes are in sm.ctx (attention_full / attention_chunk): a full layer (80 tokens) or a
// pruned one (the 16 tokens of position 4). `po` = the caller's prefetch of the first out_proj
// weight blocks. LN1 writes its output's planes into sm.h and keeps the fp32 values in registers
// (LN2's residual); FFN1 writes the hidden planes into big (features 0-127) and ctx (128-255); LN2
// writes fp32 into sm.h -- or, when the next layer's in_proj runs as split products, that layer's
// operand planes (and position 4 in fp32 to sm.ctx rows 0-15). A pruned layer after such a layer
// takes its residual from sm.ctx rows 0-15.
// Training mode (TR): the activations the backward reads are written to the workspace -- the
// attention output and the FFN hidden from their planes (the values the GEMMs consumed), the
// LayerNorm outputs from registers.
// PSX (the K7 position-split forward): a full layer for the 16 tokens of ONE window position,
// [qt, qt + 16) (column tile qt / 16, [b * 5 + s] rows), its residual in sm.h, LN2's output as planes
// for the kernel's next in_proj (ps_inproj); and K7's pruned layers take their residual from sm.h
// (PSX = 2).
// BATCH (k_value_steps): the full-width tail (80 tokens) of a layer whose in_proj ran pruned -- the
// tokens are the last positions of five consecutive windows, tile w = window w, their attention
// output's planes in sm.ctx and each lane's own residual elements in registers (`bres`, one per tile).
template <int trunk, int layer, bool last, bool TR = false, class F = NoHook, int PSX = 0, bool BATCH = false>
__device__ __forceinline__ void layer_tail(TID_F Smem& sm, const float* __restrict__ P, const TailPre& po,
                                           const TrainLayerIO& io = TrainLayerIO{}, int b0 = 0, F pre_ln2 = F{},
                                           int qt = 0, [[maybe_unused]] const f32x4* bres = nullptr) {
    constexpr int DP = kTailDepth;
    [[maybe_unused]] constexpr int tb = 8 + 16 * (trunk == 0 ? 0 : 1 + layer);  // trace slot base
    constexpr int CT = (last || PSX) ? 1 : S;
    const int t0 = last ? (S - 1) * SPW : (PSX ? qt : 0), t1 = t0 + SPW * CT;
    const float* bo = P + kOffs.o[layer_param(trunk, layer, OUTB)];
    const float* b1 = P + kOffs.o[layer_param(trunk, layer, L1B)];
    const float* b2 = P + kOffs.o[layer_param(trunk, layer, L2B)];
    constexpr int s1 = split_slot(layer_param(trunk, layer, L1W)), s2 = split_slot(layer_param(trunk, layer, L2W));
    constexpr int so = split_slot(layer_param(trunk, layer, OUTW));
    // LN2 writes the next layer's operand planes (+ position 4 in fp32 to sm.ctx rows 0-15 for the
    // full forward's pruned next layer)
    constexpr bool next_planes = !last && split_inproj<trunk, layer + 1>();
    constexpr bool row4 = next_planes && !PSX;
    constexpr bool res_ctx = split_inproj<trunk, layer>() && !PSX && !BATCH;  // the residual is in sm.ctx rows 0-15
    static_assert(!BATCH || (!last && !TR && !PSX && !next_planes), "the value pass's batched tail");
    static_assert(!res_ctx || last, "a split in_proj feeds a pruned layer");
    constexpr bool kC0 = trunk != 0 && layer == 0 && !TR && !PSX;  // trace stamps of the critic's layer-0 LNs
    const int wv = TIDX() >> 6;
    _Float16* const hp = reinterpret_cast<_Float16*>(sm.h);
    _Float16* const bp = reinterpret_cast<_Float16*>(sm.big);
    _Float16* const cp = reinterpret_cast<_Float16*>(sm.ctx);
    f32x4 h1[CT];  // LN1's output: LN2's residual
    HPre<DP> w1a;
    // the operand scales (policy_layout.hpp range table): the attention output (layer 0: one per
    // workgroup, att_sc), LN1's output, the FFN hidden units; LN2's output when it is the next layer's
    // split operand
    const OpSc s_ln1 = op_sc<trunk, layer, kOpLn1>(sm), s_hid = op_sc<trunk, layer, kOpHid>(sm);
    if constexpr (TR)  // attention output
        store_rows_planes(TID_C cp, io.o, D, 0, D, t0, b0, last, t1,
                          [&](int tok) { return att_sc<trunk, layer>(sm, tok & 15).inv; }, !PSX);
    {
        // the epilogue's bias and LN1's weight / bias ahead of the GEMM: issued after it, their L2
        // round trip (~2 k cycles with every CU reading the same lines) outlasted the partials +
        // barrier + statistics in front of their first use
        const LnPar lp = ln_load(TID_C ln_bias(TID_C bo), P + kOffs.o[layer_param(trunk, layer, N1W)],
                                 P + kOffs.o[layer_param(trunk, layer, N1B)]);
        f32x4 acc[CT];
        {  // out-projection from the attention output's planes
            f32x4 hi[CT], lo[CT];
            zero(hi);
            zero(lo);
            hgemm_tile<CT, DP>(TID_C hi, lo, po, P, so, D, 16 * wv, 0, cp, t0);
            const float att_inv = att_sc<trunk, layer>(sm, LANE() & 15).inv;  // uniform (SGPRs)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) acc[ct] = (hi[ct] + lo[ct] * kLoScale) * att_inv;
        }
        PTR(tb + 7);
        w1a = hprefetch<DP>(TID_C P, s1, D, 16 * wv, 0);
        // the LayerNorm outputs go to the workspace only for the position-split kernels (K7 reads
        // them across launches); the fused training step's weight gradients form them from x-hat
        const LnOut lo1{io.xhat1, PSX ? io.h1 : nullptr, io.rstd1, b0, last, !PSX};
        if constexpr (res_ctx) {
            const f32x4 r4[1] = {*reinterpret_cast<const f32x4*>(sm.ctx + (LANE() & 15) * LDH + 16 * wv + 4 * (LANE() >> 4))};
            residual_layernorm<CT, TR, true>(TID_C sm, acc, lp, t0, lo1, h1, r4, s_ln1.sc);
        } else {
            residual_layernorm<CT, TR, true, false, kC0 ? 55 : -1, kC0 ? 56 : -1, kC0 ? 57 : -1>(TID_C sm, acc, lp, t0, lo1, h1,
                                                                                            BATCH ? bres : nullptr, s_ln1.sc);
        }
    }
    PTR(tb + 8);
    __syncthreads();
    PTR(tb + 9);
    {  // FFN1: hidden features 0-127 -> big planes, 128-255 -> ctx planes (both free now)
        const int grow = 4 * (LANE() >> 4);
        const f32x4 ba = *reinterpret_cast<const f32x4*>(b1 + 16 * wv + grow);
        const f32x4 bb = *reinterpret_cast<const f32x4*>(b1 + 128 + 16 * wv + grow);
        f32x4 hi[CT], lo[CT];
        zero(hi);
        zero(lo);
        // FFN1's second tile's first blocks load under the first tile's last MFMAs
        HPre<DP> w1b;
        hgemm_tile<CT, DP, D / 32, LDP, kPlane, true>(TID_C hi, lo, w1a, P, s1, D, 16 * wv, 0, hp, t0, &w1b,
                                                      hfrag_ptr(TID_C P, s1, D, 128 + 16 * wv, 0));
        hstore_tile<CT, true>(TID_C hi, lo, ba, bp, 16 * wv, t0, s_ln1.inv, s_hid.sc);
        zero(hi);
        zero(lo);
        hgemm_tile<CT, DP>(TID_C hi, lo, w1b, P, s1, D, 128 + 16 * wv, 0, hp, t0);
        hstore_tile<CT, true>(TID_C hi, lo, bb, cp, 16 * wv, t0, s_ln1.inv, s_hid.sc);
    }
    const HPre<DP> w2a = hprefetch<DP>(TID_C P, s2, FF, 16 * wv, 0);
    PTR(tb + 10);
    __syncthreads();
    PTR(tb + 11);
    const HPre<DP> w2b = hprefetch<DP>(TID_C P, s2, FF, 16 * wv, 128);
    if constexpr (TR) {  // FFN hidden (post-ReLU): features 0-127 from big, 128-255 from ctx
        store_rows_planes(TID_C bp, io.u, FF, 0, D, t0, b0, last, t1, [&](int) { return s_hid.inv; }, !PSX);
        store_rows_planes(TID_C cp, io.u, FF, D, D, t0, b0, last, t1, [&](int) { return s_hid.inv; }, !PSX);
    }
    const LnPar lp2 = ln_load(TID_C ln_bias(TID_C b2), P + kOffs.o[layer_param(trunk, layer, N2W)],
                              P + kOffs.o[layer_param(trunk, layer, N2B)]);  // ahead of the GEMM, as LN1's
    f32x4 hi[CT], lo[CT];
    zero(hi);
    zero(lo);
    hgemm_tile<CT, DP>(TID_C hi, lo, w2a, P, s2, FF, 16 * wv, 0, bp, t0);
    hgemm_tile<CT, DP>(TID_C hi, lo, w2b, P, s2, FF, 16 * wv, 128, cp, t0);
    PTR(tb + 12);
    f32x4 acc2[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc2[ct] = (hi[ct] + lo[ct] * kLoScale) * s_hid.inv;
    pre_ln2();
    float ln2_sc = 1.f;
    if constexpr (next_planes) ln2_sc = op_sc<trunk, layer, kOpLn2>(sm).sc;
    residual_layernorm<CT, TR, next_planes, row4, kC0 ? 23 : -1, kC0 ? 39 : -1, kC0 ? 58 : -1>(
        TID_C sm, acc2, lp2, t0, LnOut{io.xhat2, PSX ? io.h2 : nullptr, io.rstd2, b0, last, !PSX}, nullptr, h1, ln2_sc);
    PTR(tb + 14);
}
// encoder_layer* call layer_tail through this forwarder; the K7 kernels call layer_tail itself. Not a
// second concept: the extra call level only fixes the nesting in which the compiler inlines the tail.
// Invariant: the code objects of k_policy_forward<false, ...> and k_rollout_steps depend on it -- with
// the call made directly they hold the same instructions in another order and register numbering (a
// few LayerNorm-partial address computations move). Fold it away only together with a same-box
// benchmark of those kernels.
template <int trunk, int layer, bool last, bool TR, class F = NoHook>
__device__ __forceinline__ void layer_tail_fwd(TID_F Smem& sm, const float* __restrict__ P, const TailPre& po,
                                               const TrainLayerIO& io, int b0, F pre_ln2 = F{}) {
    layer_tail<trunk, layer, last, TR, F>(TID_C sm, P, po, io, b0, pre_ln2);
}

// An encoder layer whose in_proj runs as split products: K / V of all 80 tokens and Q of the query
// tokens from the fp16 planes of the layer input, fp32 Q | K | V into sm.big, then attention and
// the layer tail. The input planes are
//   layer >= 1: in sm.h (the previous layer's LN2 wrote them, and its position-4 rows in fp32 to
//               sm.ctx rows 0-15: the residual of this pruned layer);
//   layer 0 (training forward): in sm.ctx (the embedding wrote them beside its fp32 rows in sm.h) --
//               so chunk 0's attention output waits in registers until chunk 1's GEMMs have read
//               sm.ctx, then both chunks are written.
// Lane mapping: the chunk's Q | K | V meet in sm.big and attention_task / attention_full_core read them
// with 4 lanes per task (the quad on lane bits 0-1). The value pass (k_value_steps) runs the front of its
// pruned layer 1 in the other mapping, the quad on lane bits 4-5 and no Q | K | V in sm.big
// (encoder_front_pairs below), and the tail later (layer_tail BATCH).
template <int trunk, int layer, bool last, bool TR, class F = NoHook>
__device__ __forceinline__ void encoder_layer_split(TID_F Smem& sm, const float* __restrict__ P, HPre<2> pkv,
                                                    const TrainLayerIO& io, int b0, F pre_ln2) {
    [[maybe_unused]] constexpr int tb = 8 + 16 * (trunk == 0 ? 0 : 1 + layer);  // trace slot base
    PTR(tb);
    constexpr int si = split_slot(layer_param(trunk, layer, INW));
    constexpr int CTQ = last ? 1 : S, qtok0 = last ? (S - 1) * SPW : 0;
    constexpr bool in_ctx = layer == 0;                 // the input planes: sm.ctx (layer 0) or sm.h
    static_assert(in_ctx || last, "a split in_proj after a full layer: a pruned layer");
    const float* bin = P + kOffs.o[layer_param(trunk, layer, INB)];
    const int l = LANE(), i16 = l & 15, g = l >> 4, wv = TIDX() >> 6;
    const _Float16* hp = reinterpret_cast<const _Float16*>(in_ctx ? sm.ctx : sm.h);
    TailPre po;
    [[maybe_unused]] f32x4 att0[last ? 1 : 3];  // chunk 0's attention output (in_ctx)
    [[maybe_unused]] int ti0 = 0, d00 = 0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {  // two chunks of 4 heads (LDS budget)
        HPre<2> pq;
        if (wv < 4) pq = hprefetch<2>(TID_C P, si, D, 64 * c + 16 * wv, 0);
        {  // K (waves 0-3) / V (waves 4-7) of the chunk for all 80 tokens
            const f32x4 bb = *reinterpret_cast<const f32x4*>(bin + kv_row(wv, c) + 4 * g);
            f32x4 hi[S], lo[S];
            zero(hi);
            zero(lo);
            hgemm_tile<S, 2>(TID_C hi, lo, pkv, P, si, D, kv_row(wv, c), 0, hp, 0);
            if constexpr (layer == 0) __asm__ volatile("" ::: "memory");  // the scales' LDS reads after the GEMM
            const int col = (1 + (wv >> 2)) * 64 + 16 * (wv & 3) + 4 * g;
#pragma unroll
            for (int ct = 0; ct < S; ++ct)
                *reinterpret_cast<f32x4*>(sm.big + (16 * ct + i16) * LDB + col) =
                    (hi[ct] + lo[ct] * kLoScale) * in_inv<trunk, layer>(sm, 16 * ct + i16) + bb;
        }
        if (wv < 4) {  // Q of the chunk for the query tokens (their SIMD partners did V)
            const f32x4 bq = *reinterpret_cast<const f32x4*>(bin + 64 * c + 16 * wv + 4 * g);
            f32x4 hi[CTQ], lo[CTQ];
            zero(hi);
            zero(lo);
            hgemm_tile<CTQ, 2>(TID_C hi, lo, pq, P, si, D, 64 * c + 16 * wv, 0, hp, qtok0);
            if constexpr (layer == 0) __asm__ volatile("" ::: "memory");
#pragma unroll
            for (int ct = 0; ct < CTQ; ++ct)
                *reinterpret_cast<f32x4*>(sm.big + (qtok0 + 16 * ct + i16) * LDB + 16 * wv + 4 * g) =
                    (hi[ct] + lo[ct] * kLoScale) * in_inv<trunk, layer>(sm, qtok0 + 16 * ct + i16) + bq;
        }
        if (c == 0) pkv = hprefetch<2>(TID_C P, si, D, kv_row(wv, 1), 0);
        else po = tail_prefetch<trunk, layer, last, TR>(TID_C P);
        PTR(tb + 1 + 3 * c);
        __syncthreads();
        PTR(tb + 2 + 3 * c);
        if constexpr (TR) store_qkv_chunk(TID_C sm, io.qkv, c, qtok0, b0);
        if constexpr (!in_ctx) {
            attention_chunk<trunk, layer>(TID_C sm, c, S - 1, 1, P);
        } else if constexpr (last) {  // one query position: threads < 256 own one task each
            f32x4 o;
            int ti = 0, d0 = 0;
            if (TIDX() < 4 * SPW * 4) attention_task(TID_C sm, TIDX() >> 2, S - 1, o, ti, d0);
            if (c == 0) {
                att0[0] = o;
                ti0 = ti;
                d00 = d0;
            } else if (TIDX() < 4 * SPW * 4) {
                const float asc = att_sc<trunk, layer>(sm, ti & 15).sc;
                attention_out(TID_C sm, 0, ti0, d00, att0[0], asc);
                attention_out(TID_C sm, 1, ti, d0, o, asc);
            }
        } else {
            if (c == 0) {
                attention_full_core(TID_C sm, 0, att0);
            } else {
                f32x4 o[3];
                attention_full_core(TID_C sm, 1, o);
                const float asc = att_sc<trunk, layer>(sm, (int)((TIDX() >> 4) & 15)).sc;
                attention_full_store(TID_C sm, 0, att0, asc);
                attention_full_store(TID_C sm, 1, o, asc);
            }
        }
        __syncthreads();
        PTR(tb + 3 + 3 * c);
    }
    layer_tail_fwd<trunk, layer, last, TR, F>(TID_C sm, P, po, io, b0, pre_ln2);
}

// The front of a pruned encoder_layer_split -- up to the attention output's planes in sm.ctx rows 64-79,
// the residual rows still in sm.ctx rows 0-15 -- for k_value_steps' value_front, with the chunked front's
// own GEMMs (per chunk of 4 heads one wave of a SIMD runs the K tile of a head and its Q tile, its partner
// the V tile; the same hgemm_tile calls per tile, so every token column's sums are unchanged) but without
// the trip through sm.big: an accumulator tile holds dims 4g .. 4g + 3 of sample p's five keys (or
// values) in lane (p, g), attention_head's mapping. The K wave forms the scores and the softmax weights
// in registers (attention_weights) and hands e[0..4] and 1 / sum(e) of each (head, sample) to its SIMD
// partner through 6 floats of sm.big; the V wave mixes its values with them (att_mix) and writes the
// planes. The roles swap between the chunks (chunk 0: waves 0-3 K, waves 4-7 V; chunk 1 the reverse), so
// every wave runs one K + Q + softmax and one V and mixes one chunk. Both chunks' GEMMs run back to back;
// one barrier in front of the mix and one behind it replace the four of the chunk loop.
// pkv: kv_prefetch's blocks (chunk 0's roles are encoder_layer_split's).
constexpr int kAttW = 8;  // floats per (chunk, head, sample) in sm.big: e[0..4], 1 / sum(e), pad
template <int trunk, int layer>
__device__ __forceinline__ void encoder_front_pairs(TID_F Smem& sm, const float* __restrict__ P, HPre<2> pkv) {
    static_assert(split_inproj<trunk, layer>(), "the input's planes in sm.h: a pruned layer after a full one");
    constexpr int si = split_slot(layer_param(trunk, layer, INW));
    constexpr int qtok0 = (S - 1) * SPW;
    const float* bin = P + kOffs.o[layer_param(trunk, layer, INB)];
    const int l = LANE(), i16 = l & 15, g = l >> 4, wv = TIDX() >> 6, h = wv & 3;
    const _Float16* hp = reinterpret_cast<const _Float16*>(sm.h);
    f32x4 v[S];  // the values of the chunk this wave mixes (waves 0-3: chunk 1, waves 4-7: chunk 0)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const bool kw = (wv < 4) == (c == 0);  // wave-uniform: this wave has the chunk's K, Q and softmax
        const int row = (kw ? D : 2 * D) + 64 * c + 16 * h;
        HPre<2> pq;
        if (kw) pq = hprefetch<2>(TID_C P, si, D, 64 * c + 16 * h, 0);
        f32x4 t[S];
        {
            const f32x4 bb = *reinterpret_cast<const f32x4*>(bin + row + 4 * g);
            f32x4 hi[S], lo[S];
            zero(hi);
            zero(lo);
            hgemm_tile<S, 2>(TID_C hi, lo, pkv, P, si, D, row, 0, hp, 0);
#pragma unroll
            for (int ct = 0; ct < S; ++ct)
                t[ct] = (hi[ct] + lo[ct] * kLoScale) * in_inv<trunk, layer>(sm, 16 * ct + i16) + bb;
        }
        if (kw) {
            const f32x4 bq = *reinterpret_cast<const f32x4*>(bin + 64 * c + 16 * h + 4 * g);
            f32x4 hi[1], lo[1];
            zero(hi);
            zero(lo);
            hgemm_tile<1, 2>(TID_C hi, lo, pq, P, si, D, 64 * c + 16 * h, 0, hp, qtok0);
            const f32x4 q = (hi[0] + lo[0] * kLoScale) * in_inv<trunk, layer>(sm, qtok0 + i16) + bq;
            float e[S];
            const float inv = attention_weights(TID_C sm, q, t, e);
            if (g == 0) {  // the four lanes of a quad hold the same values
                float* w = sm.big + ((c * 4 + h) * SPW + i16) * kAttW;
                *reinterpret_cast<f32x4*>(w) = f32x4{e[0], e[1], e[2], e[3]};
                *reinterpret_cast<f32x2_t*>(w + 4) = f32x2_t{e[4], inv};
            }
        } else {
#pragma unroll
            for (int ct = 0; ct < S; ++ct) v[ct] = t[ct];
        }
        if (c == 0) pkv = hprefetch<2>(TID_C P, si, D, (wv < 4 ? 2 * D : D) + 64 + 16 * h, 0);
    }
    __syncthreads();
    {
        const int c = wv < 4 ? 1 : 0;
        const float* w = sm.big + ((c * 4 + h) * SPW + i16) * kAttW;
        const f32x4 e4 = *reinterpret_cast<const f32x4*>(w);
        const f32x2_t e1 = *reinterpret_cast<const f32x2_t*>(w + 4);
        const float e[S] = {e4.x, e4.y, e4.z, e4.w, e1.x};
        f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
        att_mix(o, e, e1.y, v);
        attention_out(TID_C sm, c, qtok0 + i16, 16 * h + 4 * g, o, att_sc<trunk, layer>(sm, i16).sc);
    }
    __syncthreads();
}

// One post-LN nn.TransformerEncoderLayer (relu FFN 256, 8 heads). last: prune to column tile 4.
// Work split: 8 waves, wave w and w+4 share a SIMD (and its MFMA pipe); every GEMM gives each
// SIMD the same number of 16-row output tiles. `pkv` = the caller's prefetch of this layer's first
// K/V weight blocks. Ends WITHOUT a final barrier: the caller prefetches its next weights, then syncs.
template <int trunk, int layer, bool last, bool TR = false, class F = NoHook>
__device__ __forceinline__ void encoder_layer(TID_F Smem& sm, const float* __restrict__ P, KvPre<trunk, layer, TR> pkv,
                              const TrainLayerIO& io = TrainLayerIO{}, int b0 = 0, F pre_ln2 = F{}) {
    if constexpr (split_kv<trunk, layer, TR>()) {
        encoder_layer_split<trunk, layer, last, TR, F>(TID_C sm, P, pkv, io, b0, pre_ln2);
        return;
    } else {
    // layer 0 of the inference forward: its in_proj on the f32 MFMA from the embedding's fp32 rows
    static_assert(!TR, "the training forward's in_proj GEMMs are split products");
    [[maybe_unused]] constexpr int tb = 8 + 16 * (trunk == 0 ? 0 : 1 + layer);  // trace slot base
    PTR(tb);
    const float* Win = P + kOffs.o[layer_param(trunk, layer, INW)];
    const float* bin = P + kOffs.o[layer_param(trunk, layer, INB)];
    const int wv = TIDX() >> 6;
    constexpr int CTQ = last ? 1 : S;              // column tiles that need Q / out / LN / FFN
    constexpr int DQ = depth<CTQ>();
    constexpr int qtok0 = last ? (S - 1) * SPW : 0;

    TailPre po;
#pragma unroll
    for (int c = 0; c < 2; ++c) {  // two chunks of 4 heads (LDS budget)
        APre<DQ> pq;
        if (wv < 4) pq = prefetch<DQ>(TID_C Win, D, 64 * c + 16 * wv, 0);
        // K (waves 0-3) / V (waves 4-7) of the chunk for all 80 tokens, one 16-row tile each
        linear1<S, false, 2>(TID_C pkv, Win, D, bin, kv_row(wv, c), sm.h, LDH, 0, sm.big, LDB, (1 + (wv >> 2)) * 64 + 16 * (wv & 3), 0);
        // Q of the chunk for the query tokens, waves 0-3 (their SIMD partners did V)
        if (wv < 4) linear1<CTQ, false, DQ>(TID_C pq, Win, D, bin, 64 * c + 16 * wv, sm.h, LDH, qtok0, sm.big, LDB, 16 * wv, qtok0);
        if (c == 0) pkv = prefetch<2>(TID_C Win, D, kv_row(wv, 1), 0);
        else po = tail_prefetch<trunk, layer, last, TR>(TID_C P);
        PTR(tb + 1 + 3 * c);
        __syncthreads();
        PTR(tb + 2 + 3 * c);
        if (last) attention_chunk<trunk, layer>(TID_C sm, c, S - 1, 1, P);
        else attention_full<trunk, layer>(TID_C sm, c, P);
        __syncthreads();
        PTR(tb + 3 + 3 * c);
    }
    layer_tail_fwd<trunk, layer, last, TR, F>(TID_C sm, P, po, io, b0, pre_ln2);
    }
}

// ------------------------------------------------------------------ window-row projections
// Rollout fast path (uavhip_policy_forward_rows). Up to its in_proj, layer 0 of each trunk is
// token-local and linear after the embedding ReLU: Q|K|V of window row j at position s is
// Win (e_j + pos_s) + b_in = u_j + Win pos_s with u_j = Win e_j + b_in independent of s
// (transformer_net.py:57-63; post-LN encoder, so no norm in between). Consecutive rollout windows
// share 4 of their 5 rows (the observation deque, uav_env.py:241-242), so every env keeps the u
// rows of its current window in a 5-slot ring -- row r of the window sequence in slot r mod 5 --
// and the forward at sequence step g computes u for the new row only (slot g mod 5): the two
// layer-0 in_proj GEMMs shrink from 80 to 16 tokens per workgroup. Rows 0-3 of a window at step g
// are in slots (g + 1 + s) mod 5. Masked rows (all-zero padding, transformer_net.py:52-54) are
// keys masked in every layer and never reach the last token, so they read as zero.
// Ring row: actor K | V (2 x 128), then critic Q | K | V (3 x 128); Win pos_s table in front.
constexpr int kPposFloats = 2 * S * 3 * D;  // [trunk][s][384]
constexpr int kRowFloats = 5 * D;
struct RowIO {
    float* rp;  // [kPposFloats] Win pos_s, then ring [5][B][kRowFloats]
    int B, g;   // windows; sequence step of this forward
};
constexpr int kPwD = 4;  // in_proj k-blocks of the new-row GEMM loaded ahead (of 8)
template <int trunk> constexpr int row_parts() { return trunk == kActorTrunk ? 2 : 3; }  // K,V / Q,K,V
template <int NP>
struct RowPre {
    f32x4 v[2][2 * NP];  // per chunk: this thread's ring values of positions 0-3
    float pp[2][2];      // per chunk: this thread's share of the [5][192] Win pos_s rows
    f32x4 bias[3];       // in_proj bias of the wave's Q, K, V rows (new-row GEMM epilogue)
};

// Win pos_s of chunk c ([s][part * 64 + d], d < 64) -> registers; staged into sm.red (free during
// the chunk loop) by ppos_stage.
template <int trunk, int NP>
__device__ __forceinline__ void ppos_load(TID_F RowPre<NP>& r, const RowIO& rio) {
    const float* pp = rio.rp + (trunk == kActorTrunk ? 0 : S * 3 * D);
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = (TIDX() + NTHR * u) % (S * 192);  // (threads past 960 reload, unused)
            const int s = i / 192, rr = i - 192 * s, part = rr >> 6, cc = rr & 63;
            r.pp[c][u] = pp[s * 3 * D + part * D + 64 * c + cc];
        }
}
template <int NP>
__device__ __forceinline__ void ppos_stage(TID_F Smem& sm, const RowPre<NP>& r, int c) {
    float* pl = reinterpret_cast<float*>(sm.red);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int i = TIDX() + NTHR * u;
        if (i < S * 192) pl[i] = r.pp[c][u];
    }
}
// Item u of chunk c for this thread: float4 q of part `part` (of the NP cached parts) of token tok
// (position tok >> 4 < 4, sample tok & 15); 16 consecutive lanes read one 256-byte row segment.
template <int NP>
__device__ __forceinline__ void ring_item(TID_F int u, int& part, int& tok) {
    const int t2 = (TIDX() >> 4) + 32 * u;
    part = t2 % NP;
    tok = t2 / NP;
}
// Chunk c of the ring rows (the critic loads chunk 1 only after its new-row GEMM: registers).
template <int trunk, int NP>
__device__ __forceinline__ void ring_load(TID_F RowPre<NP>& r, const Smem& sm, const RowIO& rio, int b0, int c) {
    constexpr int ROFF = trunk == kActorTrunk ? 0 : 2 * D;
    const float* slots = rio.rp + kPposFloats;
    const int q = TIDX() & 15;
    // predicates and offsets first (LDS reads of the mask), then the loads back to back: no LDS
    // read lands in a register of an outstanding load (that forces a vmcnt(0) drain)
    int off[2 * NP];
#pragma unroll
    for (int u = 0; u < 2 * NP; ++u) {
        int part, tok;
        ring_item<NP>(TID_C u, part, tok);
        const int s = tok >> 4, p = tok & 15, b = b0 + p;
        const bool ok = b < rio.B && !sm.mask[p * S + s];
        const int slot = (rio.g + 1 + s) % 5;
        off[u] = ok ? (slot * rio.B + b) * kRowFloats + ROFF + part * D + 64 * c + 4 * q : -1;
    }
    __builtin_amdgcn_sched_barrier(0);
    // unconditional loads (masked items read ring row 0 and are dropped): a load under a branch
    // makes the compiler's vmcnt bookkeeping assume it may be missing and wait for everything
#pragma unroll
    for (int u = 0; u < 2 * NP; ++u) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(slots + (off[u] >= 0 ? off[u] : 4 * q));
        r.v[c][u] = off[u] >= 0 ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// The actor-only step's ring operands (encoder_layer_rows ONEPASS): wave wv owns head wv, and lane
// (p = lane & 15, g = lane >> 4) holds dims 4g .. 4g + 3 of sample p -- the lane mapping of the new-row
// GEMM's accumulators, so the ring rows meet the new row's Q | K | V in registers.
struct RowPre1 {
    f32x4 v[S - 1][2];  // [position 0-3][K, V]: the lane's four dims of its sample's ring rows, as loaded
    int ok;             // bit s: position s is a real row of an env in range (else v[s] reads as zero)
    f32x4 pt;           // this thread's float4 of the [5][K 128 | V 128] Win pos_s table (-> sm.red)
    f32x4 pq;           // Win pos_4 of the lane's four Q dims
    f32x4 bias[3];      // as RowPre's
};
constexpr int kPpos1Vec = S * 2 * D / 4;  // float4s of the actor's K | V table: fills sm.red exactly
static_assert(kPpos1Vec * 4 * sizeof(float) == sizeof(Smem::red) && kPpos1Vec <= NTHR, "the K | V table in sm.red");
__device__ __forceinline__ void ppos_load_head(TID_F RowPre1& r, const RowIO& rio) {
    const float* pp = rio.rp;  // the actor's rows of the table: [s][Q | K | V]
    const int i = TIDX() % kPpos1Vec;  // (threads past the table reload, unused)
    r.pt = *reinterpret_cast<const f32x4*>(pp + (i >> 6) * 3 * D + D + 4 * (i & 63));
    r.pq = *reinterpret_cast<const f32x4*>(pp + (S - 1) * 3 * D + 16 * (TIDX() >> 6) + 4 * (LANE() >> 4));
}
__device__ __forceinline__ void ppos_stage_head(TID_F Smem& sm, const RowPre1& r) {
    if (TIDX() < kPpos1Vec) reinterpret_cast<f32x4*>(sm.red)[TIDX()] = r.pt;  // [s][K 128 | V 128]
}
// ring_load for one head per wave: K and V of positions 0-3 of head wv, 8 float4 per lane, under
// ring_load's rules (predicates and offsets first, then unconditional loads back to back; a masked or
// out-of-range item reads a valid row and becomes zero). The zero is put in by the consumer (ring_value,
// from `ok`): a select here would sit inside the new-row GEMM's k-block and make it wait for the loads.
__device__ __forceinline__ void ring_load_head(TID_F RowPre1& r, const Smem& sm, const RowIO& rio, int b0) {
    const float* slots = rio.rp + kPposFloats;
    const int p = LANE() & 15, b = b0 + p;
    const int col = 16 * (int)(TIDX() >> 6) + 4 * (LANE() >> 4);
    int off[S - 1], m[S - 1];
#pragma unroll
    for (int s = 0; s < S - 1; ++s) m[s] = sm.mask[p * S + s];  // every lane, back to back: one LDS round trip
    r.ok = 0;
#pragma unroll
    for (int s = 0; s < S - 1; ++s) {
        const bool ok = (b < rio.B) & (m[s] == 0);
        const int slot = (rio.g + 1 + s) % 5;
        off[s] = ok ? (slot * rio.B + b) * kRowFloats + col : col;
        r.ok |= (int)ok << s;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < S - 1; ++s)
#pragma unroll
        for (int part = 0; part < 2; ++part) r.v[s][part] = *reinterpret_cast<const f32x4*>(slots + off[s] + part * D);
}
__device__ __forceinline__ f32x4 ring_value(const RowPre1& r, int s, int part) {
    return (r.ok >> s) & 1 ? r.v[s][part] : f32x4{0.f, 0.f, 0.f, 0.f};
}

// acc[r] += W[row[r] + i][k] . X[xtok0 + j][k] over k in [0, 128): R weight tiles against one
// activation tile (shared B operand), blocks < D from `pre` (D = KB: weights fully preloaded).
// `issued()` runs right after the last weight load is issued: loads it issues queue behind the
// GEMM's own (vmcnt retires in order), so none of the GEMM's waits cover them.
template <int R, int D, class F>
__device__ __forceinline__ void gemm_rows(TID_F f32x4 (&acc)[R], const APre<D> (&pre)[R], const float* __restrict__ W,
                                          int ldw, const int (&row)[R], const float* X, int ldx, int xtok0,
                                          F&& issued) {
    const int l = LANE(), i16 = l & 15, g = l >> 4;
    const float* xp = X + (xtok0 + i16) * ldx + 4 * g;
    f32x4 a[KB][R], b[KB];
#pragma unroll
    for (int p = 0; p < D; ++p) {
#pragma unroll
        for (int r = 0; r < R; ++r) a[p][r] = pre[r].a[p];
        b[p] = *reinterpret_cast<const f32x4*>(xp + 16 * p);
    }
#pragma unroll
    for (int i = 0; i < KB; ++i) {
        if (i + D < KB) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                a[i + D][r] = *reinterpret_cast<const f32x4*>(frag_ptr(TID_C W, ldw, row[r], 0) + 256 * (i + D));
            b[i + D] = *reinterpret_cast<const f32x4*>(xp + 16 * (i + D));
        }
        if (i == (D < KB ? KB - D - 1 : 0)) issued();
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][r][j], b[i][j], acc[r], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// gemm_rows as split products: R weight tiles of a split copy against one activation tile's planes
template <int R, int D_, class F>
__device__ __forceinline__ void hgemm_rows(TID_F f32x4 (&hi)[R], f32x4 (&lo)[R], const HPre<D_> (&pre)[R],
                                           const float* __restrict__ P, int soff, int K, const int (&row)[R],
                                           const _Float16* X, int xtok0, F&& issued) {
    constexpr int NKB = D / 32;
    const int l = LANE(), i16 = l & 15, g = l >> 4;
    const _Float16* xp = X + (xtok0 + i16) * LDP + 8 * (g ^ ((i16 >> 2) & 1));  // psw's swizzle
    f16x8 a1[NKB][R], a2[NKB][R], b1[NKB], b2[NKB];
#pragma unroll
    for (int p = 0; p < D_; ++p)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            a1[p][r] = pre[r].a1[p];
            a2[p][r] = pre[r].a2[p];
        }
    b1[0] = *reinterpret_cast<const f16x8*>(xp);
    b2[0] = *reinterpret_cast<const f16x8*>(xp + kPlane);
#pragma unroll
    for (int i = 0; i < NKB; ++i) {
        if (i + 1 < NKB) {  // B one block ahead
            b1[i + 1] = *reinterpret_cast<const f16x8*>(xp + 32 * (i + 1));
            b2[i + 1] = *reinterpret_cast<const f16x8*>(xp + 32 * (i + 1) + kPlane);
        }
        if (i + D_ < NKB) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const f16x8* wp = hfrag_ptr(TID_C P, soff, K, row[r], 0) + 128 * (i + D_);
                a1[i + D_][r] = wp[0];
                a2[i + D_][r] = wp[64];
            }
        }
        if (i == (D_ < NKB ? NKB - D_ - 1 : 0)) issued();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            hi[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[i][r], b1[i], hi[r], 0, 0, 0);
            lo[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[i][r], b2[i], lo[r], 0, 0, 0);
            lo[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[i][r], b1[i], lo[r], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}
// The new-row GEMM's weight prefetch (rows_prologue): the split copy's first blocks when layer 0's
// in_proj has one, the fp32 fragments otherwise.
template <int trunk>
constexpr bool split_ring() { return split_slot(layer_param(trunk, 0, INW)) >= 0; }
template <int trunk>
using RingPre = std::conditional_t<split_ring<trunk>(), HPre<2>, APre<kPwD>>;

// Layer 0 of a trunk on the ring: u of the new row (position 4) from `pw` (in_proj rows 128 j +
// 16 wv: this wave's Q, K and V features, all in chunk wv >> 2) and the ring rows of positions
// 0-3 from `rp`; then attention and layer_tail as in encoder_layer. Expects sm.ctx rows 64-79 =
// e of position 4 (embed_apply kEmbSplit), sm.red = Win pos_s of chunk 0 (ppos_stage).
// Q | K | V reach the attention in one of two lane mappings. Default: through sm.big, two chunks of 4
// heads, each an assembly phase, a barrier, attention_chunk / attention_full (4 lanes per task, the quad
// on lane bits 0-1) and another barrier. ONEPASS (the actor-only step, policy_block AONLY; RP = RowPre1):
// the new-row GEMM's accumulators of wave wv are Q, K and V of head wv (HD = 16) with lane (i16, g) holding
// dims 4g .. 4g + 3 of sample i16, so each wave attends for its own head in registers (attention_head, the
// quad on lane bits 4-5: the same reduction tree, see attention_task) on ring rows loaded in that mapping
// (ring_load_head) -- no assembly, no chunk loop, one barrier before the tail. It expects e of position 4
// in sm.big rows 0-15 (embed_apply kEmbOne) and the whole K | V table of Win pos_s in sm.red
// (rows_prologue_head). Every sum keeps its order: projection + bias, then + Win pos_s.
template <int trunk, bool ONEPASS = false, class RP>
__device__ __forceinline__ void encoder_layer_rows(TID_F Smem& sm, const float* __restrict__ P, const RingPre<trunk> (&pw)[3], RP& rp,
                                   const RowIO& rio, int b0) {
    constexpr bool last = trunk == kActorTrunk;  // the actor's layer 0 is its last (pruned) layer
    constexpr int NP = row_parts<trunk>();
    static_assert(std::is_same_v<RP, std::conditional_t<ONEPASS, RowPre1, RowPre<NP>>>, "the variant's ring operands");
    static_assert(!ONEPASS || (last && split_ring<trunk>()), "one pass: the actor's pruned layer, split new-row GEMM");
    constexpr int P0 = 3 - NP, ROFF = trunk == kActorTrunk ? 0 : 2 * D;
    [[maybe_unused]] constexpr int tb = 8 + 16 * (trunk == 0 ? 0 : 1);
    PTR(tb);
    const float* Win = P + kOffs.o[layer_param(trunk, 0, INW)];
    const int l = LANE(), i16 = l & 15, g = l >> 4, wv = TIDX() >> 6;
    const int rows[3] = {16 * wv, D + 16 * wv, 2 * D + 16 * wv};
    f32x4 acc[3] = {};
    auto ring_issue = [&] {
        if constexpr (ONEPASS) {
            ring_load_head(TID_C rp, sm, rio, b0);
        } else {
            ring_load<trunk>(TID_C rp, sm, rio, b0, 0);
            if (trunk == kActorTrunk) ring_load<trunk>(TID_C rp, sm, rio, b0, 1);
        }
    };
    if constexpr (split_ring<trunk>()) {  // e of position 4 as planes in sm.ctx (embed_apply kEmbSplit)
        f32x4 lo[3] = {};
        const float inv = es_factor<trunk, 1>(sm, (S - 1) * SPW + i16);  // the new row's scale
        hgemm_rows<3, 2>(TID_C acc, lo, pw, P, split_slot(layer_param(trunk, 0, INW)), D, rows,
                         reinterpret_cast<const _Float16*>(ONEPASS ? sm.big : sm.ctx), ONEPASS ? 0 : (S - 1) * SPW,
                         ring_issue);
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[j] = (acc[j] + lo[j] * kLoScale) * inv;
    } else {
        gemm_rows<3, kPwD>(TID_C acc, pw, Win, D, rows, sm.ctx, LDH, (S - 1) * SPW, ring_issue);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[j] += rp.bias[j];  // u = Win e + b
    if constexpr (!ONEPASS) {
    if (b0 + i16 < rio.B) {  // the new row -> ring slot g mod 5
        float* dst = rio.rp + kPposFloats + ((size_t)(rio.g % 5) * rio.B + b0 + i16) * kRowFloats + ROFF + 16 * wv + 4 * g;
#pragma unroll
        for (int j = P0; j < 3; ++j) *reinterpret_cast<f32x4*>(dst + (j - P0) * D) = acc[j];
    }
    }
    if constexpr (ONEPASS) {
        // One pass, one wave per head: wave wv's accumulators are Q, K and V of head wv for the 16
        // samples, lane (i16, g) holding dims 4g .. 4g + 3 of sample i16 -- attention_head's mapping, and
        // ring_load_head's. Nothing goes through sm.big and no barrier separates projection and attention;
        // the one below lets the tail's out-projection read every head's planes.
        PTR(tb + 13);
        const TailPre po = tail_prefetch<trunk, 0, last, false>(TID_C P);
        const float* pl = reinterpret_cast<const float*>(sm.red) + 16 * wv + 4 * g;  // [s][K 128 | V 128]
        f32x4 k[S], v[S];
#pragma unroll
        for (int s = 0; s < S - 1; ++s) {
            k[s] = ring_value(rp, s, 0);
            v[s] = ring_value(rp, s, 1);
        }
        k[S - 1] = acc[1];
        v[S - 1] = acc[2];
#pragma unroll
        for (int s = 0; s < S; ++s) {  // projection + bias first, then + Win pos_s
            k[s] += *reinterpret_cast<const f32x4*>(pl + s * 2 * D);
            v[s] += *reinterpret_cast<const f32x4*>(pl + s * 2 * D + D);
        }
        const f32x4 o = attention_head(TID_C sm, acc[0] + rp.pq, k, v);
        attention_out(TID_C sm, 0, (S - 1) * SPW + i16, 16 * wv + 4 * g, o, att_sc<trunk, 0>(sm, i16).sc);
        // The new row -> ring slot g mod 5, behind the attention (no load of this step reads that slot):
        // under its branch the compiler's vmcnt bookkeeping waits for everything outstanding at the next
        // use of a load -- in front of the attention that was the store's round trip on top of the loads'.
        if (b0 + i16 < rio.B) {
            float* dst = rio.rp + kPposFloats + ((size_t)(rio.g % 5) * rio.B + b0 + i16) * kRowFloats + 16 * wv + 4 * g;
            *reinterpret_cast<f32x4*>(dst) = acc[1];
            *reinterpret_cast<f32x4*>(dst + D) = acc[2];
        }
        __syncthreads();
        PTR(tb + 3);  // "attn+sync"; the other chunk-phase slots (tb + 1 .. tb + 6) are not stamped
        layer_tail_fwd<trunk, 0, last, false>(TID_C sm, P, po, TrainLayerIO{}, b0);
    } else {
    if (trunk != kActorTrunk) ring_load<trunk>(TID_C rp, sm, rio, b0, 1);
    PTR(tb + 13);
    const float* pl = reinterpret_cast<const float*>(sm.red);
    const int q = TIDX() & 15;
    TailPre po;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        // Q | K | V of the chunk -> sm.big: positions 0-3 from the ring, position 4 from acc
#pragma unroll
        for (int u = 0; u < 2 * NP; ++u) {
            int part, tok;
            ring_item<NP>(TID_C u, part, tok);
            const int bp = part + P0, s = tok >> 4;
            *reinterpret_cast<f32x4*>(sm.big + tok * LDB + bp * 64 + 4 * q) =
                rp.v[c][u] + *reinterpret_cast<const f32x4*>(pl + s * 192 + bp * 64 + 4 * q);
        }
        if ((wv >> 2) == c) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int col = 64 * j + 16 * (wv & 3) + 4 * g;
                *reinterpret_cast<f32x4*>(sm.big + ((S - 1) * SPW + i16) * LDB + col) =
                    acc[j] + *reinterpret_cast<const f32x4*>(pl + (S - 1) * 192 + col);
            }
        }
        if (c == 1) po = tail_prefetch<trunk, 0, last, false>(TID_C P);
        PTR(tb + 1 + 3 * c);
        __syncthreads();
        PTR(tb + 2 + 3 * c);
        if (c == 0) ppos_stage(TID_C sm, rp, 1);  // sm.red is read again only by the chunk-1 assembly
        if (last) attention_chunk<trunk, 0>(TID_C sm, c, S - 1, 1, P);
        else attention_full<trunk, 0>(TID_C sm, c, P);
        __syncthreads();
        PTR(tb + 3 + 3 * c);
    }
    layer_tail_fwd<trunk, 0, last, false>(TID_C sm, P, po, TrainLayerIO{}, b0);
    }
}

// Everything layer 0 of a trunk needs before its new-row GEMM (which then issues the ring loads
// behind its last weight loads): embedding operands, Win pos_s, the wave's in_proj weight tiles
// and bias. Ends with the embedding in sm.h / sm.ctx and Win pos_s of
// chunk 0 in sm.red, without a barrier.
template <int trunk, int NP, class H = NoHook>
__device__ __forceinline__ void rows_prologue(TID_F Smem& sm, const float* __restrict__ P, RingPre<trunk> (&pw)[3],
                                              RowPre<NP>& rp, const RowIO& rio, int b0, H hook = H{}) {
    const int wv = TIDX() >> 6;
    const EmbPre ep = embed_load<trunk>(TID_C P);
    ppos_load<trunk>(TID_C rp, rio);
    const float* Win = P + kOffs.o[layer_param(trunk, 0, INW)];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if constexpr (split_ring<trunk>()) pw[j] = hprefetch<2>(TID_C P, split_slot(layer_param(trunk, 0, INW)), D, j * D + 16 * wv, 0);
        else pw[j] = prefetch<kPwD>(TID_C Win, D, j * D + 16 * wv, 0);
    }
    const float* bin = P + kOffs.o[layer_param(trunk, 0, INB)];
#pragma unroll
    for (int j = 0; j < 3; ++j) rp.bias[j] = *reinterpret_cast<const f32x4*>(bin + j * D + 16 * wv + 4 * (LANE() >> 4));
    hook();  // behind the loads above: its latency overlaps theirs
    embed_apply<trunk, false, kEmbSplit>(TID_C sm, ep);
    ppos_stage(TID_C sm, rp, 0);
}
// rows_prologue of the actor-only step (encoder_layer_rows ONEPASS): the whole K | V table of Win pos_s
// goes to sm.red at once, the Q row of position 4 stays in registers, and the embedding's planes go to
// sm.big (embed_apply kEmbOne).
template <class H = NoHook>
__device__ __forceinline__ void rows_prologue_head(TID_F Smem& sm, const float* __restrict__ P,
                                                   RingPre<kActorTrunk> (&pw)[3], RowPre1& rp, const RowIO& rio,
                                                   H hook = H{}) {
    constexpr int trunk = kActorTrunk;
    const int wv = TIDX() >> 6;
    const EmbPre ep = embed_load<trunk>(TID_C P);
    ppos_load_head(TID_C rp, rio);
#pragma unroll
    for (int j = 0; j < 3; ++j) pw[j] = hprefetch<2>(TID_C P, split_slot(layer_param(trunk, 0, INW)), D, j * D + 16 * wv, 0);
    const float* bin = P + kOffs.o[layer_param(trunk, 0, INB)];
#pragma unroll
    for (int j = 0; j < 3; ++j) rp.bias[j] = *reinterpret_cast<const f32x4*>(bin + j * D + 16 * wv + 4 * (LANE() >> 4));
    hook();  // behind the loads above: its latency overlaps theirs
    embed_apply<trunk, false, kEmbOne>(TID_C sm, ep);
    ppos_stage_head(TID_C sm, rp);
}

}  // namespace pol
}  // namespace uavhip
