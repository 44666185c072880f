// policy_core.hpp -- the policy kernels' shared device primitives: constants, the LDS layout (Smem), the
// trace macros, the lane-index plumbing (TID_*), the f32 and split-product GEMM tiles, the operand range
// scales, the store tiles and the cross-lane reductions. Included by policy.hip and rollout_steps.hip
// (through the headers below it: policy_encoder.hpp, policy_block.hpp).
#pragma once
#include "common.hpp"
#include "env_device.hpp"
#include "env_group.hpp"  // (its GTR phase stamps: defined by rollout_steps.hip ahead of this header, ENVFINE builds)
#include "policy_layout.hpp"
#include "policy_train.hpp"
// The policy code is contracted (a * b + c as one fma, v_pk_fma_f32 on float pairs): the env headers
// above switch contraction off for the rest of the translation unit at file scope (their fp64 code must
// follow the reference's operation order), which until round 6 silently applied to every function
// below too. Their templates keep the state they were parsed with; the operand-range functions that
// producer and consumer must evaluate identically keep their own contract(off). Same-box A/B
// (profiles/r06u_ab_contract.txt): k_rollout_steps 49.4 -> 48.2 us per step, the training forward
// 87.6 -> 84.5 us; every -m gpu test unchanged in outcome.
#pragma clang fp contract(fast)

namespace uavhip {
namespace pol {

constexpr int SPW = 16;         // samples per workgroup
constexpr int TOK = S * SPW;    // 80
constexpr int NW = 8;            // waves per workgroup: two per SIMD
constexpr int NTHR = NW * 64;
constexpr int LDH = D + 8;      // 136: row stride = 2 mod 16 slots of 16 B -> the MFMA operand
                                // reads/writes (lane = row i + 16 * k-group g) hit 16 distinct slots
constexpr int LDB = 3 * 64 + 8; // 200: [Q 64 | K 64 | V 64] for a chunk of 4 heads
constexpr int LDX = 16;         // input rows padded 14 -> 16 (one MFMA k-block)
constexpr int LDZ = HID + 8;

typedef float f32x4 __attribute__((ext_vector_type(4)));
// make NOENV=1 (profiling builds only, wrong results): the fused rollout kernels skip the env step
// but still write the next windows -- the input windows shifted by one row, every row's constant
// feature (index 13, 1.0 in every real observation row) set -- so no position of the next step's
// windows is padding and the policy's data-dependent ring loads (a padded position reads one hot
// dummy row, ring_load) stay those of a real rollout. bench.py prices the env step as the product
// build's time minus this build's; scripts/profile_env_share.sh the same for PMC bytes. (Until round
// 4 the NOENV build left the next windows all zero -- every position but the last padded -- which also
// dropped ~41 MB per step of ring-row reads: that differential was not the env step's cost.)
#ifdef UAVHIP_EXP_NOENV
constexpr bool kExpNoEnv = true;
#else
constexpr bool kExpNoEnv = false;
#endif
// The training forward's activation stores (the rows K6 and the weight-gradient GEMM read back after
// the whole forward: Q | K | V, x-hat, the embeddings, FFN hidden units, attention outputs) are
// non-temporal: they stream past the L2 instead of evicting the weights and re-read rows there.
// Same-box A/B (profiles/r06m_train_ab_nt_stores.txt): K6 104.4-108.5 -> 101.1-101.3 us at minibatch
// 4096, the forward unchanged. Not in the position-split kernels (K7, minibatch <= 256), whose next
// launch reads the rows back from the L2 (nt there: B1 / B2 +1 us each): nt = false.
__device__ __forceinline__ void act_st(float* p, f32x4 v, bool nt = true) {
    if (nt) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
    else *reinterpret_cast<f32x4*>(p) = v;
}
typedef float f32x2_t __attribute__((ext_vector_type(2)));

// Phase tracing (make TRACE=1 only): waves 0 and 4 of the first 256 workgroups stamp s_memtime at
// the phase boundaries below; uavhip_policy_trace copies the stamps out. Off in the product build.
#if defined(UAVHIP_POLICY_TRACE)
#ifdef UAVHIP_STEPS_TU  // k_rollout_steps: its own buffer (the last step's stamps), uavhip_steps_trace
#define g_ptrace g_strace
#define g_btrace g_sbtrace
#endif
constexpr int kTraceSlots = 64;
#ifndef UAVHIP_STRACE_DEFINED
__device__ unsigned long long g_ptrace[256 * 2 * kTraceSlots];
#endif
#ifdef UAVHIP_TRACE_ALLWAVES  // make TRACE=1 TRACE_WAVES=8: all 8 waves of the first 64 workgroups
#define PTR(id)                                                                                  \
    do {                                                                                         \
        if ((tid_x() & 63) == 0 && blockIdx.x < 64)                                          \
            g_ptrace[(blockIdx.x * 8 + (tid_x() >> 6)) * kTraceSlots + (id)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define PTR(id)                                                                                  \
    do {                                                                                         \
        if ((tid_x() & 255) == 0 && blockIdx.x < 256)                                        \
            g_ptrace[(blockIdx.x * 2 + (tid_x() >> 8)) * kTraceSlots + (id)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#endif
__device__ unsigned long long g_btrace[256 * 2 * kTraceSlots];
#define BTR(id)                                                                                  \
    do {                                                                                         \
        if ((tid_x() & 255) == 0 && blockIdx.x < 256)                                        \
            g_btrace[(blockIdx.x * 2 + (tid_x() >> 8)) * kTraceSlots + (id)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define PTR(id) do {} while (0)
#define BTR(id) do {} while (0)
#endif

constexpr int kScr = NW * 3 * 64;  // backward scratch: per-wave in_proj bias partial rows
struct Smem {
    union {
        float x[TOK * LDX];     // input windows [tok = s*16 + p][k], k < 14 valid
        float scr[kScr];        // backward: scratch while the windows are not needed
    };
    float h[TOK * LDH];         // residual stream [tok][128]
    float big[TOK * LDB];       // QKV chunk / out-proj result / FFN hidden chunk
    float ctx[TOK * LDH];       // attention output / FFN output
    union {
        float z[SPW * LDZ];     // head hidden
        float2 red[NW * TOK];   // LayerNorm partials (mean, M2) per wave and token
    };
    float logits[SPW * 2];
    float value[SPW];
    int mask[SPW * S];          // key padding mask (transformer_net.py:52-54)
    float tmax[TOK];            // max_k |x_k| of each token's window row (layer 0's operand range)
    signed char es[2][TOK];     // per trunk and token: layer 0's input scale exponent s (from tmax)
    float a0f[4];               // per trunk: (2^-s, 2^s) of the workgroup's layer-0 attention output
    float rtab[28];             // the range table's static part (load_rtab, once per launch)
    float u01[SPW];             // the sampling draws, formed at the step's start (policy_block)
};
// Smem::rtab: the static operands' (2^-s, 2^s) pairs, then (14 max|W_e|, max|b_e| + max|pos|) and
// (D max|W_in|, max|b_in|) of layer 0 per trunk (policy_layout.hpp kRgOp / kRgE / kRgA0)
static_assert(kRtN <= 28 && kRgE + 4 == kRgA0, "Smem::rtab");

// Lane index plumbing. In the multi-step rollout TU (rollout_steps.hip) every forward helper takes
// the thread index as a leading parameter, laundered once per step by k_rollout_steps: the
// compiler then cannot hoist the body's lane-index arithmetic out of the step loop (where it would
// be spilled) and still shares it across the whole step. Elsewhere the macros are empty and the
// helpers read threadIdx.x as before.
#ifdef UAVHIP_STEPS_TU
#define TID_F unsigned tid_,
#define TID_C tid_,
#define TID_K (unsigned)threadIdx.x,
#define TIDX() tid_
#else
#define TID_F
#define TID_C
#define TID_K
#define TIDX() tid_x()
#endif
#define LANE() ((int)(TIDX() & (kWave - 1)))

// ------------------------------------------------------------------ GEMM building blocks
constexpr int KB = 128 / 16;

// The first D k-blocks of a single 16-row weight tile, loaded ahead of time (typically before the
// __syncthreads that precedes the GEMM: the barrier only drains LDS traffic, lgkmcnt(0), so these
// global loads stay in flight across it and their latency hides under the preceding phase).
template <int D>
struct APre {
    f32x4 a[D];
};
// GEMM weights are stored in MFMA fragment order (see kTileK): the A operand of 16-row tile
// `row / 16`, k-block kb is 1 KiB contiguous, lane l's float4 at 4 l. One wave instruction then
// reads 1 KiB of consecutive lines instead of 16 half-lines of 16 rows (3.3x the per-CU L2 rate
// measured on MI355X: scripts/micro/l2bw.hip).
__device__ __forceinline__ const float* frag_ptr(TID_F const float* W, int ldw, int row, int kw0) {
    return W + ((size_t)(row >> 4) * (ldw >> 4) + (kw0 >> 4)) * 256 + 4 * LANE();
}
template <int D>
__device__ __forceinline__ APre<D> prefetch(TID_F const float* __restrict__ W, int ldw, int row, int kw0) {
    const float* wp = frag_ptr(TID_C W, ldw, row, kw0);
    APre<D> r;
#pragma unroll
    for (int p = 0; p < D; ++p) r.a[p] = *reinterpret_cast<const f32x4*>(wp + 256 * p);
    return r;
}

// acc[ct] += W[row + i][kw0 + k] * X[xtok0 + 16 ct + j][k]  over k in [0, 128), one 16-row tile.
// Fully unrolled over the 8 k-blocks of 16; the loads of block i + D (weights from L2 as float4,
// activations from LDS as float4) are issued before the MFMAs of block i; blocks < D come from
// `pre`. Both operands use the same k permutation (k = 16 i + 4 (lane >> 4) + j for MFMA j).
template <int CT, int D, int NKB = KB>
__device__ __forceinline__ void gemm_tile(TID_F f32x4 (&acc)[CT], const APre<D>& pre, const float* __restrict__ W, int ldw,
                                          int row, int kw0, const float* X, int ldx, int xtok0) {
    const int l = LANE(), i16 = l & 15, g = l >> 4;
    const float* wp = frag_ptr(TID_C W, ldw, row, kw0);
    const float* xp[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) xp[ct] = X + (xtok0 + 16 * ct + i16) * ldx + 4 * g;
    f32x4 a[NKB], b[NKB][CT];
#pragma unroll
    for (int p = 0; p < D; ++p) {
        a[p] = pre.a[p];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) b[p][ct] = *reinterpret_cast<const f32x4*>(xp[ct] + 16 * p);
    }
#pragma unroll
    for (int i = 0; i < NKB; ++i) {
        if (i + D < NKB) {
            a[i + D] = *reinterpret_cast<const f32x4*>(wp + 256 * (i + D));
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) b[i + D][ct] = *reinterpret_cast<const f32x4*>(xp[ct] + 16 * (i + D));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][j], b[i][ct][j], acc[ct], 0, 0, 0);
        // keep the scheduler from hoisting every later block's loads (register pressure at 2
        // waves / SIMD): at most D blocks of operands are in flight
        __builtin_amdgcn_sched_barrier(0);
    }
}
template <int CT> constexpr int depth() { return CT == 1 ? 4 : 2; }

template <int CT>
__device__ __forceinline__ void zero(f32x4 (&acc)[CT]) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ------------------------------------------------------------------ split products on the f16 cores
// fp32-accurate GEMMs on v_mfma_f32_16x16x32_f16 (16 cycles per 16 x 16 x 32 block against 8 x 32
// for the f32 MFMA): both operands carried as two fp16 planes, x1 = f16(x), x2 = f16((x - x1) 2^11)
// (x1 + 2^-11 x2 = x to 2^-22 relative, the 2^11 keeps x2 out of the fp16 subnormals), and
//   W X^T = hi + 2^-11 lo,   hi += W1 X1,   lo += W1 X2 + W2 X1       (3 MFMAs per block)
// -- the dropped W2 X2 is 2^-22 of a product; the fp32 accumulation dominates the error
// (scripts/micro/split_gemm.hip: max error 0.42x the f32 MFMA's on the FFN1 shape, 3.6x faster).
// Weights: the packed buffer's split copies (policy_layout.hpp kSplitParam / kSplitOffs), blocks of
// 16 rows x 32 k = 1 KiB of w1 then 1 KiB of w2, lane l = r%16 + 16 ((k%32)/8) holding k%8.
// Activations: both planes of a token in one LDS row, [tok][plane 1: 128 halves | plane 2: 128 |
// pad 16] (plane 2 at + kPlane); lane (i16, g) reads 8 halves of token i16 per plane with one
// ds_read_b128. The 544-B rows put token i16 at bank offset 8 i16 (mod 64), conflict-free for
// ds_read_b128's lane groups (MI355X_MICROARCH.md LDS table) like the fp32 [tok][136] rows.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
constexpr int LDP = 2 * D + 16;      // halves per token row (both planes + pad)
constexpr int kPlane = D;            // plane 2 within the row
static_assert(TOK * LDP * 2 == TOK * LDH * 4 && kPlane + D <= LDP, "the two planes of an activation replace its fp32 copy");
// Offset of (token, column) in a plane image: the 16-B chunk index XOR-swizzled by bit 2 of the token,
// so the epilogues' ds_write_b64 (16 consecutive tokens per lane group) are at most 2-way conflicted
// (4-way without it) while the GEMMs' ds_read_b128 stay conflict-free
__device__ __forceinline__ int psw(int tok, int col) { return tok * LDP + (col ^ (((tok >> 2) & 1) << 3)); }
constexpr float kLoScale = 1.0f / 2048.0f;
// The LayerNorm's 1/sqrt(var + eps) and the attention's 1/sum(exp) on the hardware estimates
// (v_rsq_f32 / v_rcp_f32, about 1 ulp) instead of the correctly rounded sqrt + division sequences
// (~10 VALU each, on the LayerNorm and attention phases' dependency chains): same-box A/B
// (profiles/r06x_ab_rsq_rcp.txt) k_rollout_steps 48.6 -> 47.8 us per step, K6 101.8 -> 98.8 us, the
// training forward 85.8 -> 82.5 us; every -m gpu parity bar unchanged and green.
__device__ __forceinline__ float ln_rstd(float v) { return __builtin_amdgcn_rsqf(v); }
__device__ __forceinline__ float att_recip(float v) { return __builtin_amdgcn_rcpf(v); }
// The forward attention's score of a query against a key over a lane's 4 head dims: one packed
// multiply and one packed FMA (3 issue slots; left to itself the compiler formed 2 packed multiplies
// and 3 adds). The 1/sqrt(16) of the scores is folded into the query (kAttQ; a power of two: exact).
__device__ __forceinline__ float att_dot(const f32x4 q, const f32x4 k) {
    f32x2_t t = f32x2_t{q.x, q.y} * f32x2_t{k.x, k.y};
    t = __builtin_elementwise_fma(f32x2_t{q.z, q.w}, f32x2_t{k.z, k.w}, t);
    return t.x + t.y;
}
constexpr float kAttQ = 0.25f;  // 1/sqrt(16), on the query
// o += sum_j (e_j / den) v_j as (sum_j e_j v_j) / den: one scale of the sum instead of one per key.
// Not exp2(s log2e - mx log2e) as one FMA per score: for logits
// of 1e10 (windows at 1e5) the FMA's residual at the maximum itself is hundreds, exp2 of it inf or 0
// (NaN outputs in test_fused_forward_out_of_fp16_range_matches_torch); s - mx is exact there.
template <int N>
__device__ __forceinline__ void att_mix(f32x4& o, const float (&e)[N], float inv, const f32x4 (&v)[N]) {
    f32x4 a = e[0] * v[0];
#pragma unroll
    for (int j = 1; j < N; ++j) a += e[j] * v[j];
    o += a * inv;
}

template <int D_>
struct HPre {
    f16x8 a1[D_], a2[D_];
};
__device__ __forceinline__ const f16x8* hfrag_ptr(TID_F const float* P, int soff, int K, int row, int kw0) {
    return reinterpret_cast<const f16x8*>(P + soff) + ((size_t)(row >> 4) * (K >> 5) + (kw0 >> 5)) * 128 + LANE();
}
template <int D_>
__device__ __forceinline__ HPre<D_> hprefetch(TID_F const float* __restrict__ P, int soff, int K, int row, int kw0) {
    const f16x8* wp = hfrag_ptr(TID_C P, soff, K, row, kw0);
    HPre<D_> r;
#pragma unroll
    for (int p = 0; p < D_; ++p) {
        r.a1[p] = wp[128 * p];
        r.a2[p] = wp[128 * p + 64];
    }
    return r;
}
// hi / lo[ct] += W[row + i][kw0 + k] * X[xtok0 + 16 ct + j][k] over k in [0, 128) (4 blocks of 32):
// A blocks >= D_ loaded one block ahead of their use, B (LDS) one block ahead.
// NKB blocks of 32 k; the activation planes have rows of LDX_ halves, plane 2 at + PLX halves.
// NEXT: the blocks of the NEXT tile's prefetch (nxt, from nwp) are loaded in the last D_ iterations,
// into the registers the current tile's first blocks free there -- the next GEMM's first weight
// blocks then land under this GEMM's last MFMAs instead of after them (same register peak).
template <int CT, int D_, int NKB = D / 32, int LDX_ = LDP, int PLX = kPlane, bool NEXT = false>
__device__ __forceinline__ void hgemm_tile(TID_F f32x4 (&hi)[CT], f32x4 (&lo)[CT], const HPre<D_>& pre,
                                           const float* __restrict__ P, int soff, int K, int row, int kw0,
                                           const _Float16* X, int xtok0, HPre<D_>* nxt = nullptr,
                                           const f16x8* nwp = nullptr) {
    constexpr int kPlane = PLX;
    const int l = LANE(), i16 = l & 15, g = l >> 4;
    const f16x8* wp = hfrag_ptr(TID_C P, soff, K, row, kw0);
    const _Float16* xp[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)  // the LDP images: psw's swizzle (xtok0 is a multiple of 16)
        xp[ct] = X + (xtok0 + 16 * ct + i16) * LDX_ + (LDX_ == LDP ? 8 * (g ^ ((i16 >> 2) & 1)) : 8 * g);
    f16x8 a1[NKB], a2[NKB], b1[2][CT], b2[2][CT];
#pragma unroll
    for (int p = 0; p < D_; ++p) {
        a1[p] = pre.a1[p];
        a2[p] = pre.a2[p];
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        b1[0][ct] = *reinterpret_cast<const f16x8*>(xp[ct]);
        b2[0][ct] = *reinterpret_cast<const f16x8*>(xp[ct] + kPlane);
    }
#pragma unroll
    for (int i = 0; i < NKB; ++i) {
        const int cur = i & 1;
        if (i + D_ < NKB) {
            a1[i + D_] = wp[128 * (i + D_)];
            a2[i + D_] = wp[128 * (i + D_) + 64];
        }
        if constexpr (NEXT) {
            if (i + D_ >= NKB) {
                const int p = i - (NKB - D_);
                nxt->a1[p] = nwp[128 * p];
                nxt->a2[p] = nwp[128 * p + 64];
            }
        }
        if (i + 1 < NKB) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                b1[cur ^ 1][ct] = *reinterpret_cast<const f16x8*>(xp[ct] + 32 * (i + 1));
                b2[cur ^ 1][ct] = *reinterpret_cast<const f16x8*>(xp[ct] + 32 * (i + 1) + kPlane);
            }
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            hi[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[i], b1[cur][ct], hi[ct], 0, 0, 0);
            lo[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[i], b2[cur][ct], lo[ct], 0, 0, 0);
            lo[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[i], b1[cur][ct], lo[ct], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}
// ReLU that keeps NaN: the NaN a split operand beyond fp16's range produces (common.hpp f16_lo) must
// reach the outputs, and fmaxf(NaN, 0) = 0 (IEEE maxNum) swallowed it at the FFN and head ReLUs
// (measured: a 1.4e5 FFN activation gave finite, wrong values); same cost on the same box (r04f A/B)
__device__ __forceinline__ float relu_nan(float v) { return v < 0.f ? 0.f : v; }
// v -> its two planes at Y + psw(tok, c) (plane 2 at + kPlane): one 8-byte store per plane
// (common.hpp f16_split4: packed conversions)
__device__ __forceinline__ void hsplit_store(_Float16* Y, int o, const f32x4 v) {
    f16x4 v1, v2;
    f16_split4(v, v1, v2);
    *reinterpret_cast<f16x4*>(Y + o) = v1;
    *reinterpret_cast<f16x4*>(Y + o + kPlane) = v2;
}
// ------------------------------------------------------------------ operand ranges of the split products
// Every activation operand is split as x 2^-s and the consuming GEMM's output multiplied by 2^s
// (policy_layout.hpp range table: s = 0 on realistic weights). Static operands (LayerNorm outputs,
// FFN hidden units, the attention output of a layer >= 1) take (2^-s, 2^s) from the table; layer 0's
// input takes s per token from the token's window-row max (Smem::tmax) and layer 0's attention
// output one s per workgroup, from the max over its 16 samples' rows (Smem::a0f). Producer and
// consumer read the same s (one evaluation, kept in LDS), so both sides always agree on it.
struct OpSc {
    float sc, inv;  // 2^-s (the producer's factor), 2^s (the consumer's)
};
__device__ __forceinline__ OpSc pow2_sc(int s) { return OpSc{ldexpf(1.0f, -s), ldexpf(1.0f, s)}; }
// The scales the kernels derive from the packed table's maxima (policy_layout.hpp range_entry) ->
// Smem::rtab, once per launch before the first barrier: every later use is an LDS read, not a scalar
// load whose lgkmcnt wait would also drain the phase's LDS traffic. Waves 0-3 take 6 entries each,
// every index a compile-time constant (the maxima they need are uniform scalar loads, one round; a
// thread per entry ran every entry's branch one after another, +1 us per kernel).
template <int W>
__device__ __forceinline__ void rtab_part(TID_F Smem& sm, const float* __restrict__ M) {
#pragma unroll
    for (int j = 0; j < kRtN / 4; ++j) {
        const int i = (kRtN / 4) * W + j;
        const float v = range_entry(M, i < kRtE ? kRgOp + i : kRgE + (i - kRtE));
        if ((TIDX() & 63) == 0) sm.rtab[i] = v;
    }
}
__device__ __forceinline__ void load_rtab(TID_F Smem& sm, const float* __restrict__ P) {
    static_assert(kRtN % 4 == 0, "4 waves");
    switch (TIDX() >> 6) {  // wave-uniform
        case 0: rtab_part<0>(TID_C sm, P + kRangeOff); break;
        case 1: rtab_part<1>(TID_C sm, P + kRangeOff); break;
        case 2: rtab_part<2>(TID_C sm, P + kRangeOff); break;
        case 3: rtab_part<3>(TID_C sm, P + kRangeOff); break;
        default: break;
    }
}
// The derived table as an earlier kernel of the same step exported it (TrainIO::rtab_out: the K7
// chain's F1 derives it once per optimizer step): one plain load per entry
// instead of the maxima's scalar loads and every entry's derivation.
__device__ __forceinline__ void load_rtab_ready(TID_F Smem& sm, const float* __restrict__ rt) {
    if (TIDX() < kRtN) sm.rtab[TIDX()] = rt[TIDX()];
}
// a uniform LDS value into an SGPR (the factors are the same in every lane: no VGPR held)
__device__ __forceinline__ float rt_uniform(const Smem& sm, int i) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sm.rtab[i])));
}
template <int trunk, int layer, int kind>
__device__ __forceinline__ OpSc op_sc(const Smem& sm) {
    constexpr int op = range_op(trunk, layer, kind);
    static_assert(op >= 0, "a static operand");
    return OpSc{rt_uniform(sm, kRtOp + 2 * op), rt_uniform(sm, kRtOp + 2 * op + 1)};
}
// layer 0's input (e or e + pos) at a token whose window row has max |x_k| = m, from the trunk's
// constants ea = 14 max|W_e|, ec = max|b_e| + max|pos|; its attention output of a sample whose rows
// have max m, with a = D max|W_in|, c = max|b_in|
// (uncontracted: every site evaluates the same roundings, so a producer and its consumer agree on s)
__device__ __forceinline__ float e_bound_v(float ea, float ec, float m) {
#pragma clang fp contract(off)
    return ea * m + ec;
}
__device__ __forceinline__ OpSc e_sc_v(float ea, float ec, float m) { return pow2_sc(range_exp(e_bound_v(ea, ec, m))); }
__device__ __forceinline__ OpSc a0_sc_v(float ea, float ec, float a, float c, float m) {
#pragma clang fp contract(off)
    return pow2_sc(range_exp(a * e_bound_v(ea, ec, m) + c));
}
template <int trunk>
__device__ __forceinline__ OpSc e_sc(const Smem& sm, float m) {
    constexpr int ti = trunk_index(trunk);
    return e_sc_v(rt_uniform(sm, kRtE + 2 * ti), rt_uniform(sm, kRtE + 2 * ti + 1), m);
}
// layer 0's input scale at token tok from Smem::es (gather_windows: e_sc's exponent, evaluated once
// per token): dir -1 the producer's 2^-s, +1 the consumer's 2^s
template <int trunk, int dir>
__device__ __forceinline__ float es_factor(const Smem& sm, int tok) {
    return ldexpf(1.0f, dir * (int)sm.es[trunk_index(trunk)][tok]);
}
// The scale of an attention output (layer 0: Smem::a0f, one per workgroup -- a uniform value, held
// in SGPRs: a per-sample factor in a VGPR across the out-projection cost the rollout loop 4 VGPR
// spills; else the static one). p: the sample (unused).
template <int trunk, int layer>
__device__ __forceinline__ OpSc att_sc(const Smem& sm, int) {
    if constexpr (layer == 0) {
        constexpr int ti = trunk_index(trunk);
        return OpSc{__int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sm.a0f[2 * ti]))),
                    __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sm.a0f[2 * ti + 1])))};
    } else {
        return op_sc<trunk, layer, kOpAtt>(sm);
    }
}

// Y planes [ytok0 + 16 ct + j][ycol + i] = epi(hi + 2^-11 lo + bias[row + i])
// (the operand's scale undone: x inv; the output's planes scaled: x osc)
template <int CT, bool RELU>
__device__ __forceinline__ void hstore_tile(TID_F const f32x4 (&hi)[CT], const f32x4 (&lo)[CT], const f32x4 bb,
                                            _Float16* Y, int ycol, int ytok0, float inv, float osc) {
    const int l = LANE(), i16 = l & 15, g = l >> 4;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        f32x4 v = (hi[ct] + lo[ct] * kLoScale) * inv + bb;
        if (RELU) {
            v.x = relu_nan(v.x); v.y = relu_nan(v.y); v.z = relu_nan(v.z); v.w = relu_nan(v.w);
        }
        hsplit_store(Y, psw((ytok0 + 16 * ct + i16), ycol + 4 * g), v * osc);
    }
}

// Y[ytok0 + 16 ct + j][ycol + i] = epi(acc + bias[brow + i]); lane (j, g) holds rows 4g..4g+3
template <int CT, bool RELU>
__device__ __forceinline__ void store_tile(TID_F const f32x4 (&acc)[CT], const f32x4 bb, float* Y, int ldy, int ycol,
                                           int ytok0) {
    const int l = LANE(), i16 = l & 15, g = l >> 4;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        f32x4 v = acc[ct] + bb;
        if (RELU) {
            v.x = relu_nan(v.x); v.y = relu_nan(v.y); v.z = relu_nan(v.z); v.w = relu_nan(v.w);
        }
        *reinterpret_cast<f32x4*>(Y + (ytok0 + 16 * ct + i16) * ldy + ycol + 4 * g) = v;
    }
}

// One 16-row output tile per wave: Y[tok][ycol + i] = epi(W[row + i] . X[tok]^T + b[row + i]).
// The bias is loaded ahead of the k-loop, so the epilogue does not wait one more L2 round trip.
template <int CT, bool RELU, int D>
__device__ __forceinline__ void linear1(TID_F const APre<D>& pre, const float* W, int ldw, const float* bias, int row,
                                        const float* X, int ldx, int xtok0, float* Y, int ldy, int ycol, int ytok0) {
    const f32x4 bb = *reinterpret_cast<const f32x4*>(bias + row + 4 * (LANE() >> 4));
    f32x4 acc[CT];
    zero(acc);
    gemm_tile<CT, D>(TID_C acc, pre, W, ldw, row, 0, X, ldx, xtok0);
    store_tile<CT, RELU>(TID_C acc, bb, Y, ldy, ycol, ytok0);
}

// ------------------------------------------------------------------ VALU pieces
// Cross-lane sums without the LDS crossbar (__shfl_xor lowers to ds_bpermute on gfx950):
// DPP quad permutes inside a quad, v_permlane16/32_swap across rows / halves. Both lanes of a
// pair compute the same a + b, so the results are bitwise equal across the group.
__device__ __forceinline__ float add_xor1(float v) {
    return v + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));  // [1,0,3,2]
}
__device__ __forceinline__ float add_xor2(float v) {
    return v + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));  // [2,3,0,1]
}
__device__ __forceinline__ float add_xor16(float v) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float add_xor32(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// max over each row of 16 lanes (quad permutes, then row_ror 4 / 8), the same in every lane of the row
template <int ctrl>
__device__ __forceinline__ float max_dpp(float v) {
    return fmaxf(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), ctrl, 0xF, 0xF, true)));
}
__device__ __forceinline__ float row16_max(float v) {
    return max_dpp<0x128>(max_dpp<0x124>(max_dpp<0x4E>(max_dpp<0xB1>(v))));
}
// max over the wave (the same value in every lane)
__device__ __forceinline__ float wave_max(float v) {
    v = row16_max(v);
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

}  // namespace pol
}  // namespace uavhip
