// rollout_steps.hip -- k_rollout_steps (uavhip_rollout_steps): the fused rollout step (policy_block.hpp)
// in a loop over the steps of one launch, compiled in a translation unit of its own so that every
// lane-index expression can be laundered per use (UAVHIP_TID_LAUNDER, common.hpp tid_x(); UAVHIP_STEPS_TU,
// policy_core.hpp TID_*) without touching the code of the single-step kernels. k_decode_steps
// (uavhip_decode_steps), the actor-only inference loop, lives here for the same reason, and so do
// k_rollout_actor_steps / k_value_steps (uavhip_rollout_actor_steps, uavhip_value_steps), the rollout
// with the critic off the step chain. policy.hip's C entry points reach the kernels through the four
// launch_* functions declared in policy_steps.hpp and defined here.
#define UAVHIP_STEPS_TU 1
#define UAVHIP_TID_LAUNDER 1
#include "common.hpp"
#include "env_device.hpp"
#if defined(UAVHIP_POLICY_TRACE) && defined(UAVHIP_ENV_FINE)
// make TRACE=1 ENVFINE=1 (k_rollout_steps only): stamps inside the grouped env step (env_group.hpp
// GTR, slots 40-47) in the same buffer as PTR, waves 0 and 4 of the first 256 workgroups
namespace uavhip { namespace pol { __device__ unsigned long long g_strace[256 * 2 * 64]; } }
#define UAVHIP_STRACE_DEFINED 1
#define GTR(id)                                                                                  \
    do {                                                                                         \
        if ((tid_x() & 255) == 0 && blockIdx.x < 256)                                        \
            ::uavhip::pol::g_strace[(blockIdx.x * 2 + (tid_x() >> 8)) * 64 + (id)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#endif
#include "policy_steps.hpp"

namespace uavhip {
namespace pol {

// A multi-step kernel's view of its arguments (struct Args, its only parameter) for one step: `a`, read
// through a kernarg pointer laundered here, so the loads sit where the body uses them instead of being
// hoisted out of the loop and kept live (spilled) across the whole body; pointers loaded from the
// constant address space are still known global. With it `bx` = blockIdx.x and `tid`, the forward
// helpers' lane index (TID_F), both opaque per step; the mask restores threadIdx.x's range, which the
// launder hides from the compiler. A macro: the text of the block, nothing the compiler could treat otherwise.
#define UAVHIP_KARGS(Args)                                       \
    typedef const __attribute__((address_space(4))) Args* kargs; \
    kargs ka = (kargs)__builtin_amdgcn_kernarg_segment_ptr();    \
    int bx = blockIdx.x;                                         \
    unsigned tid = threadIdx.x;                                  \
    asm volatile("" : "+s"(ka), "+s"(bx), "+v"(tid));            \
    tid &= NTHR - 1;                                             \
    const Args& a = *(const Args*)ka

// Launch the instantiation of a fused step kernel for the env path of args.env over args.B envs: two
// envs per wave wherever every wave's envs come in pairs (policy_block's env_grp for all of them), the
// grouped path alone; else the one-env-per-wave path alone (bitwise the same steps).
template <auto KGrp, auto KWave, class Args>
int launch_env_path(const Args& args, const char* name, hipStream_t stream) {
    const dim3 grid((args.B + SPW - 1) / SPW), block(NTHR);
    if (args.env.N <= envgrp::L && args.env.M <= envgrp::L && args.B % 2 == 0)
        hipLaunchKernelGGL(KGrp, grid, block, 0, stream, args);
    else
        hipLaunchKernelGGL(KWave, grid, block, 0, stream, args);
    return check_launch(name);
}

template <int ENVP>  // kEnvGrp / kEnvWave (launch_env_path picks)
__global__ __launch_bounds__(NTHR) void k_rollout_steps(const StepsArgs args) {
    __shared__ __attribute__((aligned(16))) Smem sm;
    if (threadIdx.x >= NTHR / 2) __builtin_amdgcn_s_setprio(1);
    if (threadIdx.x == 0) g_tid_zero = 0;
    load_rtab(TID_K sm, args.P);  // the weights are the launch's: once
    for (int t = 0; t < args.seq.n; ++t) {
        __syncthreads();  // g_tid_zero; the previous step's LDS scratch and global stores
        UAVHIP_KARGS(StepsArgs);
        const size_t o = (size_t)t * a.B;
        const RowIO r{a.rio.rp, a.rio.B, a.rio.g + t};
        const EnvOut e{a.eo.auto_reset, a.eo.obs + t * a.seq.obs_stride, a.eo.rew + o, a.eo.done + o,
                       a.eo.info ? a.eo.info + o * UAVHIP_INFO_COUNT : nullptr};
        policy_block<false, true, ENVP>(tid, sm, a.P, a.states + t * a.seq.obs_stride, a.B, nullptr, a.seed,
                                        a.offset + t * a.seq.off_stride, a.offset_dev, a.action_out + o, a.logp_out + o,
                                        a.value_out + o, nullptr, nullptr, TrainIO{}, r, a.env, e, bx);
    }
}
#ifdef UAVHIP_POLICY_TRACE
extern "C" int uavhip_steps_trace(unsigned long long* out, int n) {  // the last step's k_rollout_steps stamps
    return copy_trace(g_ptrace, 256 * 2 * kTraceSlots, out, n);
}
#endif
int launch_rollout_steps(const StepsArgs& sa, hipStream_t stream) {
    return launch_env_path<k_rollout_steps<kEnvGrp>, k_rollout_steps<kEnvWave>>(sa, "k_rollout_steps", stream);
}

// Decode (uavhip_decode_steps): k_rollout_steps' loop with the actor-only block (policy_block AONLY)
// and UAVHIP_STEP_HOLD -- a finished env waits, untouched, and the workgroup leaves the loop once its
// 16 envs are finished. The windows ping-pong between the two slots of obs2; nothing is kept per
// step but the optional action trace. Wave 0's first 16 lanes keep each env's step count, return
// and finished flag in LDS between the steps (one lane per env; the step's reward and done flag
// come back through global memory, args.ep_return / args.finished, behind a workgroup barrier).
// After a step: the envs' counters (wave 0's first 16 lanes), the trace row and the workgroup's
// all-finished flag. The arguments are read through a kernarg pointer of its own, so that nothing
// of the step's stays live across the forward for it.
__device__ __forceinline__ void post_step(unsigned tid, Smem& sm, int t, double* s_ret, int* s_cnt, int* s_fin,
                                          int* s_all) {
    typedef const __attribute__((address_space(4))) DecodeArgs* kargs;
    kargs ka = (kargs)__builtin_amdgcn_kernarg_segment_ptr();
    int bx = blockIdx.x;
    asm volatile("" : "+s"(ka), "+s"(bx));
    const DecodeArgs& a = *(const DecodeArgs*)ka;
    if (tid < SPW) {
        const int p = tid, e = bx * SPW + p;
        bool fin = true;
        if (e < a.B) {
            const bool was = s_fin[p] != 0;
            if (!was) {
                s_cnt[p] += 1;
                if (a.ep_return) s_ret[p] = s_ret[p] + a.ep_return[e];  // this step's reward
            }
            if (a.actions) a.actions[(size_t)t * a.B + e] = was ? (int8_t)-1 : (int8_t)sm.mask[p];
            fin = was || a.finished[e] != 0;
            s_fin[p] = fin;
        }
        const unsigned m = (unsigned)ballot(fin) & 0xffffu;
        if (p == 0) *s_all = m == 0xffffu;
    }
}
template <int ENVP>
__global__ __launch_bounds__(NTHR) void k_decode_steps(const DecodeArgs args) {
    __shared__ __attribute__((aligned(16))) Smem sm;
    __shared__ double s_ret[SPW];
    __shared__ int s_cnt[SPW], s_fin[SPW], s_all;
    if (threadIdx.x >= NTHR / 2) __builtin_amdgcn_s_setprio(1);
    if (threadIdx.x == 0) g_tid_zero = 0;
    load_rtab(TID_K sm, args.P);
    if (threadIdx.x < SPW) {
        const int p = threadIdx.x, e = blockIdx.x * SPW + p;
        const bool fin = e >= args.B || args.env.istate[(long long)e * UAVHIP_IST_COUNT + UAVHIP_IST_UAV_IDX] >= args.env.N;
        s_fin[p] = fin;
        s_cnt[p] = 0;
        s_ret[p] = (e < args.B && args.ep_return) ? args.ep_return[e] : 0.0;
        const unsigned m = (unsigned)ballot(fin) & 0xffffu;
        if (p == 0) s_all = m == 0xffffu;
    }
    int t = 0;
    for (;;) {
        __syncthreads();  // s_all; g_tid_zero; the previous step's LDS scratch and global stores
        UAVHIP_KARGS(DecodeArgs);
        // workgroup-uniform: every wave reads the flag wave 0 wrote before the barrier
        if (__builtin_amdgcn_readfirstlane(s_all) || t >= a.n_max) break;
        const int slot = (a.rio.g + t) & 1;
        const RowIO r{a.rio.rp, a.rio.B, a.rio.g + t};
        const EnvOut eo{UAVHIP_STEP_HOLD, a.obs2 + (slot ^ 1) * a.obs_stride, a.ep_return, a.finished, nullptr};
        policy_block<false, true, ENVP, false, true>(tid, sm, a.P, a.obs2 + slot * a.obs_stride, a.B, nullptr, a.seed,
                                                     a.offset + t * a.off_stride, a.offset_dev, nullptr, nullptr,
                                                     nullptr, nullptr, nullptr, TrainIO{}, r, a.env, eo, bx,
                                                     a.greedy_stride);
        __syncthreads();  // the env step's reward / done stores; sm.mask still holds the actions
        post_step(tid, sm, t, s_ret, s_cnt, s_fin, &s_all);
        ++t;
    }
    // the envs' totals; the trace rows the workgroup did not run (the arguments through a kernarg
    // pointer of their own again: loaded here, not kept from the prologue across the loop)
    UAVHIP_KARGS(DecodeArgs);
    const int e0 = bx * SPW;
    if (tid < SPW && e0 + (int)tid < a.B) {
        const int p = tid, e = e0 + p;
        a.steps[e] += s_cnt[p];
        a.finished[e] = s_fin[p] != 0;
        if (a.ep_return) a.ep_return[e] = s_ret[p];
    }
    if (a.actions) {
        for (int i = tid; i < (a.n_max - t) * SPW; i += NTHR) {
            const int e = e0 + i % SPW;
            if (e < a.B) a.actions[(size_t)(t + i / SPW) * a.B + e] = -1;
        }
    }
}
int launch_decode_steps(const DecodeArgs& da, hipStream_t stream) {
    return launch_env_path<k_decode_steps<kEnvGrp>, k_decode_steps<kEnvWave>>(da, "k_decode_steps", stream);
}

// Rollout with the critic taken off the step chain (uavhip_rollout_actor_steps + uavhip_value_steps).
// Sampling and the env step read the actor's logits only; the value of a window is read by the GAE
// alone, after the launch. k_rollout_actor_steps is k_rollout_steps' loop over the actor-only block
// (policy_block AONLY, as k_decode_steps but with the rollout's auto-reset, sampling for every env
// and the trajectory outputs): every window, action, logp, reward, done, info row, the env state and
// the actor's ring rows are bitwise k_rollout_steps'; no value is written and the critic's ring rows
// are not touched. k_value_steps then walks the recorded windows obs[0 .. n] with the critic alone, on
// the critic's ring rows (below): the values are bitwise k_rollout_steps'.
template <int ENVP>
__global__ __launch_bounds__(NTHR) void k_rollout_actor_steps(const StepsArgs args) {
    __shared__ __attribute__((aligned(16))) Smem sm;
    if (threadIdx.x >= NTHR / 2) __builtin_amdgcn_s_setprio(1);
    if (threadIdx.x == 0) g_tid_zero = 0;
    load_rtab(TID_K sm, args.P);
    for (int t = 0; t < args.seq.n; ++t) {
        __syncthreads();  // g_tid_zero; the previous step's LDS scratch and global stores
        UAVHIP_KARGS(StepsArgs);
        const size_t o = (size_t)t * a.B;
        const RowIO r{a.rio.rp, a.rio.B, a.rio.g + t};
        const EnvOut e{a.eo.auto_reset, a.eo.obs + t * a.seq.obs_stride, a.eo.rew + o, a.eo.done + o,
                       a.eo.info ? a.eo.info + o * UAVHIP_INFO_COUNT : nullptr};
        policy_block<false, true, ENVP, false, true, 1>(tid, sm, a.P, a.states + t * a.seq.obs_stride, a.B, nullptr,
                                                     a.seed, a.offset + t * a.seq.off_stride, a.offset_dev,
                                                     a.action_out + o, a.logp_out + o, nullptr, nullptr, nullptr,
                                                     TrainIO{}, r, a.env, e, bx, 0);
    }
}
int launch_rollout_actor_steps(const StepsArgs& sa, hipStream_t stream) {  // sa.value_out is not read
    return launch_env_path<k_rollout_actor_steps<kEnvGrp>, k_rollout_actor_steps<kEnvWave>>(sa, "k_rollout_actor_steps",
                                                                                          stream);
}

// k_value_steps: the windows in groups of kVG consecutive steps (the last group may be shorter). Per
// window, value_front runs the critic up to layer 1's attention exactly as the value-only block
// does -- layer 0 on the ring rows, layer 1's K | V GEMM, the last token's attention -- and stashes
// the 16 attention-output rows (their fp16 planes) and the 16 residual rows (fp32) of the window in
// the workgroup's slice of `stash` (LDS is full; the slice, 85 KB, stays in the L2). Layer 1's
// out-projection, LN1, FFN1, FFN2, LN2 and the value head, which the per-step kernels run on one
// 16-token tile per step with every weight streamed from the L2 for it, then run once per group on
// the kVG x 16 stashed tokens as full 80-token tiles (layer_tail BATCH: tile w = window w). Every
// token's sums are formed in the per-step order, so the values are bitwise k_rollout_steps'.
// No workgroup reads what another wrote; every barrier is in workgroup-uniform control flow (the
// group sizes derive from the kernel's arguments alone).
constexpr int kStashVec = 2 * SPW * LDH / 4;  // float4s per window: planes rows, then residual rows
static_assert(LDP * 2 == LDH * 4, "a planes row and an fp32 row are the same bytes");
__device__ __forceinline__ void value_front(TID_F Smem& sm, const float* __restrict__ P, const float* __restrict__ states,
                                            int B, const RowIO& rio, int b0, f32x4* __restrict__ st) {
    PTR(0);
    gather_windows<false, true>(TID_C sm, states, B, TrainIO{}, b0, false, P + kRangeOff);
    __syncthreads();
    PTR(1);
    a0f_from_tmax(TID_C sm);
    {
        RingPre<kCriticTrunk> pw[3];
        RowPre<3> rp;
        rows_prologue<kCriticTrunk>(TID_C sm, P, pw, rp, rio, b0);
        PTR(2);
        __syncthreads();
        encoder_layer_rows<kCriticTrunk>(TID_C sm, P, pw, rp, rio, b0);
    }
    // layer 1's front: the chunked GEMMs, the last token's attention in their registers
    const KvPre<kCriticTrunk, 1, false> pkv = kv_prefetch<kCriticTrunk, 1, false>(TID_C P);
    __syncthreads();
    encoder_front_pairs<kCriticTrunk, 1>(TID_C sm, P, pkv);
    // the attention output's planes (sm.ctx rows 64-79) and the residual rows (sm.ctx rows 0-15, fp32)
    PTR(3);
    const f32x4* cx = reinterpret_cast<const f32x4*>(sm.ctx);
    for (int i = TIDX(); i < kStashVec; i += NTHR) {
        const int h = kStashVec / 2;
        st[i] = i < h ? cx[(S - 1) * SPW * LDH / 4 + i] : cx[i - h];
    }
    PTR(4);
}
// The value head's first layer (128 -> 64, ReLU) on the batched tail's 80 tokens: sm.h -> z rows in
// sm.big (free after FFN2), feature tile wv & 3 of CT token tiles from tok0 (waves 0-3: tiles 0-2,
// waves 4-7: tiles 3-4, so both waves of a SIMD work). Per token the sums are head_mlp's.
template <int CT>
__device__ __forceinline__ void value_head_gemm(TID_F Smem& sm, const float* __restrict__ P, const APre<KB>& pw, int tok0) {
    const int row = 16 * ((TIDX() >> 6) & 3);
    linear1<CT, true, KB>(TID_C pw, P + kOffs.o[kCriticHead + 0], D, P + kOffs.o[kCriticHead + 1], row, sm.h, LDH, tok0,
                         sm.big, LDZ, row, tok0);
}
__global__ __launch_bounds__(NTHR) void k_value_steps(const ValueArgs args) {
    __shared__ __attribute__((aligned(16))) Smem sm;
    if (threadIdx.x >= NTHR / 2) __builtin_amdgcn_s_setprio(1);
    if (threadIdx.x == 0) g_tid_zero = 0;
    load_rtab(TID_K sm, args.P);
    const int nt = args.n + (args.last_values ? 1 : 0);  // workgroup-uniform (kernel arguments)
    for (int t0 = 0; t0 < nt; t0 += kVG) {
        for (int w = 0; w < kVG && t0 + w < nt; ++w) {
            __syncthreads();  // g_tid_zero; the previous window's LDS reads and ring-row stores
            UAVHIP_KARGS(ValueArgs);
            const int t = t0 + w;
            const RowIO r{a.rio.rp, a.rio.B, a.rio.g + t};
            value_front(tid, sm, a.P, a.obs + t * a.obs_stride, a.B, r, bx * SPW,
                        reinterpret_cast<f32x4*>(a.stash) + ((size_t)bx * kVG + w) * kStashVec);
        }
        __syncthreads();  // the stash stores (read back by other lanes); sm.ctx is rewritten
        UAVHIP_KARGS(ValueArgs);
        const int gw = min(kVG, nt - t0), b0 = bx * SPW;
        PTR(5);
        // tile w <- window w: the planes to sm.ctx (every load issued before the first LDS store;
        // unconditional, clamped loads), each lane's own residual elements to registers -- their round
        // trip hides under the out-projection. The plane tiles of a short group are zero; their residual
        // is whatever the stash holds (tokens are independent and those tiles' values are not written).
        f32x4 res[kVG];
        {
            const f32x4* st = reinterpret_cast<const f32x4*>(a.stash) + (size_t)bx * kVG * kStashVec;
            constexpr int h = kStashVec / 2, kAll = kVG * h, kIt = (kAll + NTHR - 1) / NTHR;
            f32x4* cx = reinterpret_cast<f32x4*>(sm.ctx);
            f32x4 v[kIt];
#pragma unroll
            for (int u = 0; u < kIt; ++u) {
                const int i = min((int)tid + u * NTHR, kAll - 1), w = i / h;
                v[u] = st[w * kStashVec + (i - w * h)];
            }
            const int ro = h + (tid & 15) * (LDH / 4) + 4 * (tid >> 6) + ((tid >> 4) & 3);
#pragma unroll
            for (int w = 0; w < kVG; ++w) res[w] = st[w * kStashVec + ro];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < kIt; ++u) {
                const int i = tid + u * NTHR;
                if (i < kAll) cx[i] = i / h < gw ? v[u] : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        const TailPre po = tail_prefetch<kCriticTrunk, 1, false, false>(tid, a.P);
        PTR(6);
        __syncthreads();
        layer_tail<kCriticTrunk, 1, false, false, NoHook, 0, true>(tid, sm, a.P, po, TrainLayerIO{}, b0, NoHook{}, 0, res);
        // the value head on the 80 tokens: first layer on the MFMA, second on the VALU (16 lanes per
        // token, head_mlp's sums), its operands loaded ahead of the barriers
        const int wv = tid >> 6, k4 = tid & 15;
        const APre<KB> ph = prefetch<KB>(tid, a.P + kOffs.o[kCriticHead + 0], D, 16 * (wv & 3), 0);  // the whole tile
        const f32x4 w2 = *reinterpret_cast<const f32x4*>(a.P + kOffs.o[kCriticHead + 2] + 4 * k4);
        const float bb2 = a.P[kOffs.o[kCriticHead + 3]];
        __syncthreads();
        if (wv < 4) value_head_gemm<3>(tid, sm, a.P, ph, 0);
        else value_head_gemm<2>(tid, sm, a.P, ph, 3 * SPW);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < (TOK * 16 + NTHR - 1) / NTHR; ++r) {
            const int tok = (NTHR / 16) * r + (tid >> 4);
            if (tok < TOK) {  // wave-uniform
                const f32x4 z = *reinterpret_cast<const f32x4*>(sm.big + tok * LDZ + 4 * k4);
                float acc = (w2.x * z.x + w2.y * z.y) + (w2.z * z.z + w2.w * z.w);
                acc = add_xor2(add_xor1(acc));
                acc += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(acc), 0x141, 0xF, 0xF, true));  // row_half_mirror
                acc += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(acc), 0x140, 0xF, 0xF, true));  // row_mirror
                const int w = tok / SPW, b = b0 + (tok & (SPW - 1)), t = t0 + w;
                if (k4 == 0 && w < gw && b < a.B) (t < a.n ? a.values + (size_t)t * a.B : a.last_values)[b] = acc + bb2;
            }
        }
        PTR(7);
    }
}
int launch_value_steps(const ValueArgs& va, hipStream_t stream) {
    hipLaunchKernelGGL(k_value_steps, dim3((va.B + SPW - 1) / SPW), dim3(NTHR), 0, stream, va);
    return check_launch("k_value_steps");
}

}  // namespace pol
}  // namespace uavhip
