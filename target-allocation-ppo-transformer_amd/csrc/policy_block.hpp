// policy_block.hpp -- one workgroup's whole forward of its 16 samples: the heads, the categorical, the loss
// terms, the window gather, policy_block (+ the fused env step) and the single-step kernel
// k_policy_forward. Included by policy.hip and rollout_steps.hip.
#pragma once
#include "policy_encoder.hpp"

namespace uavhip {
namespace pol {

// 128 -> 64 (MFMA, waves 0-3) -> relu -> nout (VALU) on the last-position rows (transformer_net.py:77-91)
// (XT: the rows' first token in sm.h; k_value_steps' batched tail has five tiles of them)
template <int head, int nout, int DQ = 4, int XT = (S - 1) * SPW>
__device__ void head_mlp(TID_F Smem& sm, const float* __restrict__ P, const APre<DQ>& pw, float* out) {
    const float* W0 = P + kOffs.o[head + 0];
    const float* b0 = P + kOffs.o[head + 1];
    const float* W2 = P + kOffs.o[head + 2];
    const float* b2 = P + kOffs.o[head + 3];
    const int wv = TIDX() >> 6;
    // second layer: 16 lanes per (sample p, output a) = item p * nout + a, 4 hidden features per
    // lane; its weights and bias are loaded before the first layer's GEMM
    constexpr int kItems = SPW * nout;
    const int item = TIDX() >> 4, k4 = TIDX() & 15;
    const int p = item / nout, a = (item - p * nout) % nout;  // in range for every thread
    const f32x4 w2 = *reinterpret_cast<const f32x4*>(W2 + a * HID + 4 * k4);
    const float bb2 = b2[a];
    if (wv < HID / 16) linear1<1, true, DQ>(TID_C pw, W0, D, b0, 16 * wv, sm.h, LDH, XT, sm.z, LDZ, 16 * wv, 0);
    __syncthreads();
    if (item < kItems) {  // wave-uniform: kItems * 16 is a multiple of 64
        const f32x4 z = *reinterpret_cast<const f32x4*>(sm.z + p * LDZ + 4 * k4);
        float acc = (w2.x * z.x + w2.y * z.y) + (w2.z * z.z + w2.w * z.w);
        acc = add_xor2(add_xor1(acc));
        acc += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(acc), 0x141, 0xF, 0xF, true));  // row_half_mirror
        acc += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(acc), 0x140, 0xF, 0xF, true));  // row_mirror
        if (k4 == 0) out[item] = acc + bb2;
    }
    __syncthreads();
}

// Categorical(softmax(logits)) as torch.distributions evaluates it (transformer_net.py:124-144):
// p = softmax(l); p /= sum(p); lc = log(clamp(p, eps, 1 - eps)); logp = lc[a]; ent = -sum(lc * p).
struct CatVals {
    float y0, y1, s, p0, p1, c0, c1, lc0, lc1;
};
__device__ __forceinline__ CatVals categorical(float l0, float l1) {
    CatVals c;
    const float m = fmaxf(l0, l1);
    const float e0 = expf(l0 - m), e1 = expf(l1 - m);
    const float den = e0 + e1;
    c.y0 = e0 / den;
    c.y1 = e1 / den;
    c.s = c.y0 + c.y1;
    c.p0 = c.y0 / c.s;
    c.p1 = c.y1 / c.s;
    const float eps = 1.1920928955078125e-07f;
    c.c0 = fminf(fmaxf(c.p0, eps), 1.f - eps);
    c.c1 = fminf(fmaxf(c.p1, eps), 1.f - eps);
    c.lc0 = logf(c.c0);
    c.lc1 = logf(c.c1);
    return c;
}

// Training mode: relu(head.0) rows of the 16 samples (sm.z) -> z [Bm][64].
__device__ __forceinline__ void store_hidden(TID_F const Smem& sm, float* __restrict__ z, int b0) {
    if (TIDX() < SPW * HID / 4) {
        const int p = TIDX() / (HID / 4), q = TIDX() % (HID / 4);
        *reinterpret_cast<f32x4*>(z + (size_t)(b0 + p) * HID + 4 * q) =
            *reinterpret_cast<const f32x4*>(sm.z + p * LDZ + 4 * q);
    }
}

// Training mode: per-sample PPO loss terms of ppo.py:148-160 (Categorical as torch evaluates it,
// transformer_net.py:124-144) and their workgroup sums in sample order -> fpart[blk][4];
// logits / value -> smp[b][5..7] for the backward.
// One sample's four terms from its smp row o[0..4] (action, old logp, old value, return, advantage)
// and its logits / value -> t[4].
__device__ __forceinline__ void loss_terms(const float (&o)[5], float l0, float l1, float v, float eps_clip,
                                           float* t, float* verr = nullptr) {
    const CatVals c = categorical(l0, l1);
    const float logp = o[0] > 0.f ? c.lc1 : c.lc0;
    const float ratio = expf(logp - o[1]);
    const float A = o[4];
    const float s1 = ratio * A;
    const float s2 = fminf(fmaxf(ratio, 1.f - eps_clip), 1.f + eps_clip) * A;
    const float R = o[3], ov = o[2];
    const float vc = ov + fminf(fmaxf(v - ov, -eps_clip), eps_clip);
    const bool pad = o[0] < 0.f;  // padding row (idx < 0): no loss terms
    t[0] = pad ? 0.f : fminf(s1, s2);
    t[1] = pad ? 0.f : (v - R) * (v - R);
    t[2] = pad ? 0.f : (vc - R) * (vc - R);
    t[3] = pad ? 0.f : -(c.lc0 * c.p0 + c.lc1 * c.p1);
    // the largest value error itself (its square overflows fp32 from |v - R| ~ 1.8e19 on: ADVICE r05)
    if (verr) *verr = pad ? 0.f : fmaxf(fabsf(v - R), fabsf(vc - R));
}
// the block's sums in sample order (threads 0-3, one term each) -> fpart[blk][4]; thread 4: the
// block's largest value error max(|v - R|, |vc - R|) (red[4 SPW + i], loss_terms' verr) -> vpart[blk]
// (the critic backward's gradient scale, heads_bwd)
__device__ __forceinline__ void loss_block_sums(TID_F const float* red, float* fpart, float* vpart, int blk) {
    if (TIDX() < 4) {
        float acc = 0.f;
        for (int i = 0; i < SPW; ++i) acc += red[4 * i + TIDX()];
        fpart[blk * 4 + TIDX()] = acc;
    } else if (TIDX() == 4 && vpart) {
        float m = 0.f;
        for (int i = 0; i < SPW; ++i) m = fmaxf(m, red[4 * SPW + i]);
        vpart[blk] = m;
    }
}
__device__ void loss_partials(TID_F Smem& sm, const TrainIO& io, int b0) {
    float* red = sm.x;  // free after the embeddings
    if (TIDX() < SPW) {
        const int p = TIDX();
        float* o = io.smp + (size_t)(b0 + p) * 8;  // o[0..4] written by this thread at kernel start
        const float l0 = sm.logits[2 * p], l1 = sm.logits[2 * p + 1], v = sm.value[p];
        o[5] = l0;
        o[6] = l1;
        o[7] = v;
        const float eps_clip = hyper_f32(io.hyper, UAVHIP_HP_EPS_CLIP, io.eps_clip);
        const float oi[5] = {o[0], o[1], o[2], o[3], o[4]};
        loss_terms(oi, l0, l1, v, eps_clip, red + 4 * p, red + 4 * SPW + p);
    }
    __syncthreads();
    loss_block_sums(TID_C red, io.fpart, io.vpart, b0 / SPW);
}

// The 16 windows of a workgroup -> sm.x[tok = s*16 + p][k], k padded 14 -> 16 with zeros (batch
// tail zero-filled) and the key padding mask -> sm.mask; training mode gathers minibatch row idx[b]
// of the trajectory buffer (idx < 0: a padding row, computed on row 0 and flagged by action -1 in
// smp, so it adds nothing to the loss or gradients) and, if `writer`, stores the windows, the mask
// and the per-sample loss inputs into the workspace. Ends without a barrier.
template <bool TR, bool RING = false>  // RING: only position 4's exponents are read (the new row's)
__device__ __forceinline__ void gather_windows(TID_F Smem& sm, const float* __restrict__ states, int B, const TrainIO& io,
                                               int b0, bool do_actor, const float* __restrict__ rg) {
    {   // <= 3 elements per thread, every load of a round issued before any is used: the
        // training gather is two dependent rounds (row index, then window / loss inputs)
        constexpr int kEl = (TOK * LDX + NTHR - 1) / NTHR;
        size_t src[kEl];
#pragma unroll
        for (int u = 0; u < kEl; ++u) {
            const int i = TIDX() + u * NTHR, p = (i / LDX) % SPW;
            src[u] = (size_t)(b0 + p);
            if (TR && i < TOK * LDX) src[u] = (size_t)max(io.idx[b0 + p], 0);
        }
        size_t ssrc = 0;
        [[maybe_unused]] bool pad = false;
        if (TR && TIDX() < SPW) {
            const int r = io.idx[b0 + TIDX()];
            pad = r < 0;
            ssrc = (size_t)max(r, 0);
        }
        float v[kEl];
#pragma unroll
        for (int u = 0; u < kEl; ++u) {
            const int i = TIDX() + u * NTHR;
            const int t = i / LDX, k = i - t * LDX, s = t / SPW, p = t - s * SPW;
            v[u] = (i < TOK * LDX && k < IN && b0 + p < B) ? states[(src[u] * S + s) * IN + k] : 0.f;
        }
        float ld[5];
        if (TR && TIDX() < SPW) {  // per-sample loss inputs
            ld[0] = pad ? -1.f : (float)(io.act_in[ssrc] != 0);
            ld[1] = io.oldlp_in[ssrc];
            ld[2] = io.oldv_in[ssrc];
            ld[3] = io.ret_in[ssrc];
            ld[4] = io.adv_in[ssrc];
        }
#pragma unroll
        for (int u = 0; u < kEl; ++u) {
            const int i = TIDX() + u * NTHR;
            {  // key padding mask (all-zero rows, the last never masked) from the registers: the 16
               // lanes of a token row vote; and the row's max |x_k| (layer 0's operand range)
                static_assert(LDX == 16 && NTHR % LDX == 0, "one token row = 16 lanes");
                const unsigned long long nz = __ballot(v[u] != 0.f);
                const float rmax = row16_max(fabsf(v[u]));
                if (i < TOK * LDX && (i % LDX) == 0) {
                    const int t = i / LDX, s = t / SPW, p = t - s * SPW;
                    const bool m = (s < S - 1) && ((nz >> (LANE() & 48)) & 0xFFFFull) == 0;
                    sm.mask[p * S + s] = m;
                    sm.tmax[t] = rmax;
                    // element u's rows start at token u NTHR / LDX: the ring forward needs position 4 only
                    if (!RING || (u * NTHR) / LDX >= (S - 1) * SPW)
#pragma unroll
                    for (int ti = 0; ti < 2; ++ti)  // layer 0's constants from the table's maxima (rg)
                        sm.es[ti][t] = (signed char)range_exp(
                            e_bound_v(range_entry(rg, kRgE + 2 * ti), range_entry(rg, kRgE + 2 * ti + 1), rmax));
                    if (TR && do_actor) {
                        io.mask[(size_t)(b0 + p) * S + s] = m ? 1.f : 0.f;
                        io.tmax[(size_t)(b0 + p) * S + s] = rmax;
                    }
                }
            }
            if (i >= TOK * LDX) continue;
            sm.x[i] = v[u];
            if (TR && do_actor) io.xg[(size_t)trow(i / LDX, b0) * 16 + (i % LDX)] = v[u];
        }
        if (TR && do_actor && TIDX() < SPW) {
            float* o = io.smp + (size_t)(b0 + TIDX()) * 8;
            for (int c = 0; c < 5; ++c) o[c] = ld[c];
        }
    }
}

// The workgroup's layer-0 attention-output scale per trunk (Smem::a0f) from the max over its 80
// window rows (rows 0..TOK-1 of m, one float each): wave 0, once the rows are visible; read behind
// a later barrier. The bound holds for every sample of the workgroup. e / a0: layer 0's constants
// (policy_layout.hpp kRgE / kRgA0: Smem::rtab, or a0f_consts of the table's maxima).
// (a0f_load: wave 0's two rows per lane, issued early; a0f_finish: the reduction and the factors)
__device__ __forceinline__ float a0f_load(TID_F const float* m) {
    static_assert(TOK <= 128, "two rows per lane");
    const int l = TIDX();
    return l < 64 ? fmaxf(m[l], l + 64 < TOK ? m[l + 64] : 0.f) : 0.f;
}
// returns the workgroup's max (wave 0 only; 0 elsewhere)
__device__ __forceinline__ float a0f_finish(TID_F Smem& sm, float v, const float* e, const float* a0) {
    if (TIDX() < 64) {
        const int l = TIDX();
        v = wave_max(v);
        if (l < 2) {
            const OpSc f = a0_sc_v(e[2 * l], e[2 * l + 1], a0[2 * l], a0[2 * l + 1], v);
            sm.a0f[2 * l] = f.sc;
            sm.a0f[2 * l + 1] = f.inv;
        }
        return v;
    }
    return 0.f;
}
__device__ __forceinline__ float a0f_from_max(TID_F Smem& sm, const float* m, const float* e, const float* a0) {
    return a0f_finish(TID_C sm, a0f_load(TID_C m), e, a0);
}
__device__ __forceinline__ float a0f_from_tmax(TID_F Smem& sm) {
    return a0f_from_max(TID_C sm, sm.tmax, sm.rtab + kRtE, sm.rtab + kRtA0);
}

// Fused rollout step (uavhip_rollout_step): the env step of the sampled actions (uav_env.py:295-435)
// after the forward, on the same workgroup's 16 envs.
struct EnvOut {
    int auto_reset;
    float* obs;     // [E][5][14] next windows (f32, or binary16 under UAVHIP_ENV_OBS_F16)
    double* rew;    // [E]
    uint8_t* done;  // [E]
    double* info;   // [E][UAVHIP_INFO_COUNT] (nullable)
};

// ROWS: layer 0 of both trunks on the window-row projection ring (inference only).
// ENV: the env step of the sampled actions follows (needs ROWS; envs b0 .. b0 + 15): a bit mask of
// the env-step code compiled in -- kEnvGrp (two envs per wave, N, M <= 32, both envs of every wave in
// range), kEnvWave (one env per wave, any N, M <= 64), both (chosen per wave at run time). The
// one-launch rollout instantiates one path per launch (71 -> 58.5 KB of code, 28 -> 9 VGPR spills).
enum { kEnvGrp = 1, kEnvWave = 2, kEnvBoth = 3 };
// One workgroup's whole forward (+ env step) of its 16 samples; the kernels below wrap it.
// VONLY (inference, ROWS): the critic trunk and head only -- the value of each window, nothing
// else (the rollout's bootstrap V(s_T), uavhip_policy_value_rows); the actor's ring row of the step
// is not written.
// AONLY (inference, ROWS, ENV): the mirror image, the actor trunk and head only and then the env step
// (k_decode_steps) -- the critic's ring rows are neither read nor written, no value; env b decodes
// greedily (a = l1 > l0) iff greedy_stride > 0 and b % greedy_stride == 0, else it samples. Its pruned
// layer attends in the projection's registers, one wave per head (encoder_layer_rows ONEPASS): bitwise
// the two-chunk path's outputs and ring rows.
// ETAG: the env step's instantiation tag (envdev::step_once TAG; 1 in k_rollout_actor_steps).
template <bool TR, bool ROWS, int ENV, bool VONLY = false, bool AONLY = false, int ETAG = 0>
__device__ __forceinline__ void policy_block(TID_F Smem& sm, const float* __restrict__ P, const float* __restrict__ states,
                                             int B, const int8_t* __restrict__ actions_in, uint64_t seed,
                                             uint64_t offset, const uint64_t* __restrict__ offset_dev,
                                             int8_t* __restrict__ action_out, float* __restrict__ logp_out,
                                             float* __restrict__ value_out, float* __restrict__ ent_out,
                                             float* __restrict__ logits_out, const TrainIO& io, const RowIO& rio,
                                             const uavhip_env& env, const EnvOut& eo, int bx,
                                             [[maybe_unused]] int greedy_stride = 0) {
    static_assert(!(TR && ROWS), "the training forward recomputes every row");
    static_assert(!ENV || ROWS, "the fused env step follows the rollout forward");
    static_assert(!VONLY || (ROWS && !ENV && !TR), "value only: the inference ring forward");
    static_assert(!AONLY || (ROWS && ENV && !TR && !VONLY), "actor only: the inference ring forward + env step");
    // training trunk split (TrainIO::split): role 1 = actor trunk + head, 2 = critic trunk + head
    // of sample block blk; role 0 = both (the rollout always)
    int blk = bx, role = VONLY ? 2 : AONLY ? 1 : 0;
    if constexpr (TR) {
        if (io.split) {
            role = blk < io.split ? 1 : 2;
            if (role == 2) blk -= io.split;
        }
    }
    const bool do_actor = role != 2, do_critic = role != 1;
    const int b0 = blk * SPW;
    // training forward without the trunk split (TrainIO::mix): every other group of 8 workgroups
    // runs the critic trunk first, so the two trunks' HBM-heavy activation stores and compute phases
    // overlap across the chip (as K6's BwdIO::mix)
    [[maybe_unused]] bool critic_first = false;
    if constexpr (TR) critic_first = role == 0 && io.mix && ((blk >> 3) & 1);
    PTR(0);
    // training mode: the first trunk's embedding operands and first K/V weight blocks are loaded
    // before the minibatch gather stores its rows (a load behind a store burst waits for the burst)
    [[maybe_unused]] EmbPre ep_a, ep_c;
    [[maybe_unused]] KvPre<kActorTrunk, 0, TR> pkv_a;
    [[maybe_unused]] KvPre<kCriticTrunk, 0, TR> pkv_c;
    if constexpr (TR) {
        if (do_actor && !critic_first) {
            ep_a = embed_load<kActorTrunk>(TID_C P);
            pkv_a = kv_prefetch<kActorTrunk, 0, TR>(TID_C P);
        } else {
            ep_c = embed_load<kCriticTrunk>(TID_C P);
            pkv_c = kv_prefetch<kCriticTrunk, 0, TR>(TID_C P);
        }
    }
    gather_windows<TR, ROWS>(TID_C sm, states, B, io, b0, do_actor, P + kRangeOff);
    // the sampling's Philox draws (a counter function of the sample's index alone) by the last wave's
    // first lanes while the windows load, so that the serial tail after the heads (one wave's
    // sampling) no longer runs the 10 Philox rounds
    if constexpr (!TR) {
        const int pd = (int)TIDX() - (NTHR - kWave);
        if (!actions_in && pd >= 0 && pd < SPW) {
            const unsigned long long c = offset + (offset_dev ? *offset_dev : 0ull) + (unsigned long long)(b0 + pd);
            const u32x4 r = philox(u32x4{(uint32_t)c, (uint32_t)(c >> 32), 0x5eedu, 0x9e37u}, (uint32_t)seed,
                                   (uint32_t)(seed >> 32));
            sm.u01[pd] = u01f(r.x);
            // actor only: a greedy env's draw is the sentinel -1 (u01f is never negative); decided
            // here, where greedy_stride need not stay live across the forward
            if constexpr (AONLY) {
                if (greedy_stride > 0 && (b0 + pd) % greedy_stride == 0) sm.u01[pd] = -1.f;
            }
        }
    }
    __syncthreads();
    PTR(1);
    // layer 0's attention-output scales, read behind the next barrier (the ring forward: once the
    // actor's prologue loads are issued, so that wave 0's reduction overlaps their round trip)
    if (!ROWS || !do_actor) {
        const float xm = a0f_from_tmax(TID_C sm);
        if (TR && TIDX() == 0 && io.xmax) io.xmax[blk] = xm;  // the block's range for the weight gradients
    }
    // the training forward exports its derived scales for the weight-gradient GEMM (TrainIO::rtab_out)
    if (TR && blk == 0 && TIDX() < kRtN && io.rtab_out) io.rtab_out[TIDX()] = sm.rtab[TIDX()];
    const int wv = TIDX() >> 6;
    const float* headw_a = P + kOffs.o[kActorHead];
    const float* headw_c = P + kOffs.o[kCriticHead];
    // fused env step (ENV): two envs per wave side by side, state loads issued before the critic head
    // (AONLY: before the actor head)
    [[maybe_unused]] const bool env_grp =
        (ENV & kEnvGrp) && env.N <= envgrp::L && env.M <= envgrp::L && b0 + 2 * wv + 1 < B;
    [[maybe_unused]] envgrp::GRegs gR;
    [[maybe_unused]] envgrp::GPending gq;
    // actor trunk (1 layer) + head
    if constexpr (ROWS) {
        if constexpr (AONLY) {  // the actor-only step: attention in the projection's registers
            RingPre<kActorTrunk> pw[3];
            RowPre1 rp;
            rows_prologue_head(TID_C sm, P, pw, rp, rio, [&] { a0f_from_tmax(TID_C sm); });
            PTR(2);
            __syncthreads();
            encoder_layer_rows<kActorTrunk, true>(TID_C sm, P, pw, rp, rio, b0);
        } else if (do_actor) {
            RingPre<kActorTrunk> pw[3];
            RowPre<2> rp;
            rows_prologue<kActorTrunk>(TID_C sm, P, pw, rp, rio, b0, [&] { a0f_from_tmax(TID_C sm); });
            PTR(2);
            __syncthreads();
            encoder_layer_rows<kActorTrunk>(TID_C sm, P, pw, rp, rio, b0);
        }
    }
    // training mode: the actor head's and the critic embedding's / first GEMM's operands are loaded
    // ahead of the actor's LN2 activation stores (layer_tail hook)
    // the head's weight prefetch depth: the training forward holds two blocks (four spilled one,
    // reloaded behind the activation store burst)
    constexpr int kHd = TR ? 2 : 4;
    APre<kHd> ph;
    // the training forward's actor (a lambda: TrainIO::mix calls it after the critic in half the
    // workgroups); the inference forward keeps its inline block below (the same code as before the
    // mix: as a lambda, its register allocation changed and the NOENV build of k_rollout_steps went
    // from 3 to 11 VGPR spills, skewing the env-step differential)
    [[maybe_unused]] auto actor = [&] {
        if constexpr (TR && !ROWS) {
            // the split layer-0 in_proj reads the embedding's planes in sm.ctx
            embed_apply<kActorTrunk, TR, kEmbH, split_kv<kActorTrunk, 0, TR>()>(TID_C sm, ep_a, io.e[0],
                                                                                           nullptr, b0);
            PTR(2);
            __syncthreads();
            auto hook = [&] {
                if (wv < 4) ph = prefetch<kHd>(TID_C headw_a, D, 16 * wv, 0);
                if (do_critic && !critic_first) {
                    ep_c = embed_load<kCriticTrunk>(TID_C P);
                    pkv_c = kv_prefetch<kCriticTrunk, 0, TR>(TID_C P);
                }
            };
            encoder_layer<kActorTrunk, 0, true, TR, decltype(hook)>(TID_C sm, P, pkv_a, io.L[0], b0, hook);
            __syncthreads();
            PTR(3);
            head_mlp<kActorHead, 2, kHd>(TID_C sm, P, ph, sm.logits);
            store_hidden(TID_C sm, io.z[0], b0);  // before the critic's LayerNorm partials reuse sm.z
        }
    };
    if constexpr (TR) {
        if (do_actor && !critic_first) actor();
    } else if (do_actor) {
        if constexpr (!ROWS) {
            APre<2> pkv = prefetch<2>(TID_C P + kOffs.o[layer_param(kActorTrunk, 0, INW)], D, kv_row(wv, 0), 0);
            embed<kActorTrunk, TR>(TID_C sm, P, io.e[0], nullptr, b0);
            PTR(2);
            __syncthreads();
            encoder_layer<kActorTrunk, 0, true, TR>(TID_C sm, P, pkv, io.L[0], b0);
        }
        // actor only: the env step's state loads land while the actor head runs
        if constexpr (AONLY && (ENV & kEnvGrp) && !kExpNoEnv) {
            if (env_grp) {
                const int le = tid_env() & 63;
                envgrp::gload_issue(gR, gq, env, b0 + 2 * (int)(tid_env() >> 6) + (le >> 5), le & 31);
            }
        }
        if (wv < 4) ph = prefetch<kHd>(TID_C headw_a, D, 16 * wv, 0);
        __syncthreads();
        PTR(3);
        head_mlp<kActorHead, 2, kHd>(TID_C sm, P, ph, sm.logits);
    }  // do_actor
    PTR(4);
    if (do_critic) {
        // critic trunk (2 layers) + head
        if constexpr (ROWS) {
            RingPre<kCriticTrunk> pw[3];
            RowPre<3> rp;
            rows_prologue<kCriticTrunk>(TID_C sm, P, pw, rp, rio, b0);
            __syncthreads();
            encoder_layer_rows<kCriticTrunk>(TID_C sm, P, pw, rp, rio, b0);
        }
        KvPre<kCriticTrunk, 1, TR> pkv;
        if constexpr (!ROWS) {
            if constexpr (TR) {
                embed_apply<kCriticTrunk, TR, kEmbH, split_kv<kCriticTrunk, 0, TR>()>(TID_C sm, ep_c, io.e[1],
                                                                                                 nullptr, b0);
                __syncthreads();
                auto hook = [&] { pkv = kv_prefetch<kCriticTrunk, 1, TR>(TID_C P); };
                encoder_layer<kCriticTrunk, 0, false, TR, decltype(hook)>(TID_C sm, P, pkv_c, io.L[1], b0, hook);
            } else {
                APre<2> pkv0 = prefetch<2>(TID_C P + kOffs.o[layer_param(kCriticTrunk, 0, INW)], D, kv_row(wv, 0), 0);
                embed<kCriticTrunk, TR>(TID_C sm, P, io.e[1], nullptr, b0);
                __syncthreads();
                encoder_layer<kCriticTrunk, 0, false, TR>(TID_C sm, P, pkv0, io.L[1], b0);
            }
        }
        if constexpr (!TR) pkv = kv_prefetch<kCriticTrunk, 1, TR>(TID_C P);
        __syncthreads();
        if constexpr (TR) {
            auto hook = [&] {
                if (wv < 4) ph = prefetch<kHd>(TID_C headw_c, D, 16 * wv, 0);
            };
            encoder_layer<kCriticTrunk, 1, true, TR, decltype(hook)>(TID_C sm, P, pkv, io.L[2], b0, hook);
        } else {
            encoder_layer<kCriticTrunk, 1, true, TR>(TID_C sm, P, pkv, io.L[2], b0);
        }
        // the env step's state loads land while the critic head runs
        if constexpr ((ENV & kEnvGrp) && !kExpNoEnv) {
            if (env_grp) {
                const int le = tid_env() & 63;
                envgrp::gload_issue(gR, gq, env, b0 + 2 * (int)(tid_env() >> 6) + (le >> 5), le & 31);
            }
        }
        if (!TR && wv < 4) ph = prefetch<kHd>(TID_C headw_c, D, 16 * wv, 0);
        __syncthreads();
        PTR(5);
        head_mlp<kCriticHead, 1, kHd>(TID_C sm, P, ph, sm.value);
        PTR(6);
        if (TR) store_hidden(TID_C sm, io.z[1], b0);
    }  // do_critic
    if constexpr (TR) {
        if (critic_first) {  // the actor's operands now (not prefetched: the critic's hooks are full)
            ep_a = embed_load<kActorTrunk>(TID_C P);
            pkv_a = kv_prefetch<kActorTrunk, 0, TR>(TID_C P);
            __syncthreads();  // the actor's trunk reuses the critic's buffers (sm.z after store_hidden)
            actor();
        }
    }
    if (TR) {
        if (role == 0) {
            loss_partials(TID_C sm, io, b0);
        } else if (TIDX() < SPW) {  // trunk split: this trunk's head outputs -> smp[5..7]
            float* o = io.smp + (size_t)(b0 + TIDX()) * 8;
            if (do_actor) {
                o[5] = sm.logits[2 * TIDX()];
                o[6] = sm.logits[2 * TIDX() + 1];
            } else {
                o[7] = sm.value[TIDX()];
            }
        }
        return;
    }
    if constexpr (VONLY) {  // the value alone
        if (TIDX() < SPW && b0 + (int)TIDX() < B) value_out[b0 + TIDX()] = sm.value[TIDX()];
        return;
    }
    // Categorical(softmax(logits)): sample / log_prob / entropy (transformer_net.py:118-122)
    if (TIDX() < SPW) {
        const int p = TIDX(), b = b0 + p;
        if (b < B) {
            const float l0 = sm.logits[2 * p], l1 = sm.logits[2 * p + 1];
            const float m = fmaxf(l0, l1);
            const float lse = m + logf(expf(l0 - m) + expf(l1 - m));
            const float lp0 = l0 - lse, lp1 = l1 - lse;
            const float p0 = expf(lp0), p1 = expf(lp1);
            int a;
            if (actions_in) {
                a = actions_in[b] != 0;
            } else {
                const float u = sm.u01[p];  // drawn at the step's start
                a = u < p0 ? 0 : 1;
                if constexpr (AONLY) {  // greedy decode (the draw's sentinel): torch.argmax (a tie gives 0)
                    if (u < 0.f) a = l1 > l0;
                }
            }
            if (action_out) action_out[b] = (int8_t)a;
            if (logp_out) logp_out[b] = a ? lp1 : lp0;
            if (ent_out) ent_out[b] = -(p0 * lp0 + p1 * lp1);
            if (value_out) value_out[b] = sm.value[p];
            if (logits_out) { logits_out[2 * b] = l0; logits_out[2 * b + 1] = l1; }
            if (ENV) sm.mask[p] = a;  // the key mask is dead after the forward
        }
    }
    PTR(7);
    if constexpr (ENV && kExpNoEnv) {  // NOENV: the next windows without the env step (timing only)
        __syncthreads();
        for (int i = TIDX(); i < SPW * envdev::kObs; i += NTHR) {
            const int p = i / envdev::kObs, r = i - p * envdev::kObs, s_ = r / IN, k = r - s_ * IN;
            const int e = b0 + p;
            const float v = sm.x[((s_ < S - 1 ? s_ + 1 : S - 1) * SPW + p) * LDX + k];
            if (e < B) envdev::obs_at(eo.obs, e, false)[r] = k == IN - 1 ? 1.0f : v;
        }
    }
    if constexpr (ENV && !kExpNoEnv) {
        // UAVEnv.step of this workgroup's 16 envs, two per wave (one env per wave at a time,
        // envdev::step_once on register state; the wave's row scratch in the dead sm.x). Both envs'
        // registers are loaded in one round before either steps.
        __syncthreads();
        PTR(60);
        using namespace envdev;
        const int lane = tid_env() & 63, wve = tid_env() >> 6, e0 = b0 + 2 * wve;
        if constexpr ((ENV & kEnvGrp) != 0) if (env_grp) {
            // both envs side by side, 32 lanes each (env_group.hpp); window scratch in the dead sm.h
            const int j = lane & 31, g = lane >> 5, e = e0 + g;
            envgrp::GRegs& R = gR;
            R.tab = nullptr;
            R.win = sm.h + (2 * wve + g) * envgrp::kWin;
            envgrp::gload_finish(R, gq, env, e, j);
            PTR(61);
            envgrp::gstep<false, AONLY, ETAG>(R, env, e, j, sm.mask[2 * wve + g], eo.auto_reset, obs_at(eo.obs, e, obs_f16(env)),
                          (AONLY && !eo.rew) ? nullptr : eo.rew + e,  // the decode's return is optional
                          eo.done + e, eo.info ? eo.info + (size_t)e * UAVHIP_INFO_COUNT : nullptr);
            PTR(62);
            envgrp::gstore_delta(R, env, e, j);  // only the entries the step changed
            PTR(63);
        }
        if constexpr ((ENV & kEnvWave) != 0) if (!env_grp && e0 < B) {
            const bool two = e0 + 1 < B;
            EnvRegs<1> R0, R1;
            R0.row = R1.row = sm.x + 16 * wve;
            load_regs<1, true>(R0, env, e0, lane);
            if (two) load_regs<1, true>(R1, env, e0 + 1, lane);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (k == 1 && !two) break;
                EnvRegs<1>& R = k ? R1 : R0;
                const int e = e0 + k;
                step_once<1, false, AONLY, ETAG>(R, env, e, lane, sm.mask[2 * wve + k], eo.auto_reset,
                                    obs_at(eo.obs, e, obs_f16(env)), (AONLY && !eo.rew) ? nullptr : eo.rew + e,
                                    eo.done + e,
                                    eo.info ? eo.info + (size_t)e * UAVHIP_INFO_COUNT : nullptr);
                store_regs(R, env, e, lane);
            }
        }
    }
}

template <bool TR, bool ROWS = false, int ENV = 0, bool VONLY = false>
__global__ __launch_bounds__(NTHR) void k_policy_forward(const float* __restrict__ P, const float* __restrict__ states,
                                                         int B, const int8_t* __restrict__ actions_in, uint64_t seed,
                                                         uint64_t offset, const uint64_t* __restrict__ offset_dev,
                                                         int8_t* __restrict__ action_out,
                                                         float* __restrict__ logp_out, float* __restrict__ value_out,
                                                         float* __restrict__ ent_out, float* __restrict__ logits_out,
                                                         const TrainIO io, const RowIO rio, const uavhip_env env,
                                                         const EnvOut eo) {
    __shared__ __attribute__((aligned(16))) Smem sm;
    // the younger half (waves 4-7, the arbitration loser of every phase) at priority 1
    if (tid_x() >= NTHR / 2) __builtin_amdgcn_s_setprio(1);
    load_rtab(TID_K sm, P);
    policy_block<TR, ROWS, ENV, VONLY>(TID_K sm, P, states, B, actions_in, seed, offset, offset_dev, action_out, logp_out,
                                       value_out, ent_out, logits_out, io, rio, env, eo, blockIdx.x);
}

}  // namespace pol
}  // namespace uavhip
