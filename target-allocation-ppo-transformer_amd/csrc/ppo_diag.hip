// ppo_diag.hip -- update diagnostics of a PPO batch (uavhip_ppo_diagnostics, include/uavhip.h):
// approximate KL, clip fractions, ratio statistics, explained variance and a non-finite count from the
// old / new log-probabilities and values and the returns. The fused training step (train.hip) reports
// the three losses only; these are what tell a healthy update from a collapsing one.
//
// Pattern of k_adv_partials / k_adv_normalize (gae.hip): per-block fp64 partials reduced in a fixed
// order, then one block that merges them in index order -- no atomics, bitwise repeatable, capturable.
// The variances carry (count, mean, M2) and merge with the pairwise update formula (Chan et al.), never
// sum(x^2) - sum(x)^2 / n: constant returns give a variance of exactly 0. fp contraction off: every
// product and sum rounds once, as the numpy restatement in tests/test_gpu_ppo_diag.py does.
#include "common.hpp"

#pragma clang fp contract(off)

namespace uavhip {
namespace {
constexpr int kDiagBlock = 256;      // threads per block
constexpr int kDiagMaxBlocks = 256;  // partials at most (the finishing block stages them all in LDS)
constexpr int kDiagWaves = kDiagBlock / kWave;
// one partial: the running sums of a block, kDiagSlots doubles
enum { kPKl = 0, kPRsum, kPClip, kPVclip, kPNonfin, kPRmax, kPCnt, kPMeanX, kPM2X, kPMeanY, kPM2Y, kPPad, kDiagSlots };

struct DiagAcc {
    double kl, rsum, clip, vclip, nonfin, rmax;  // sums, counts (exact in fp64) and the ratio's maximum
    double cnt, mx, m2x, my, m2y;                // (count, mean, M2) of x = R - V_old and of y = R
};

__device__ __forceinline__ DiagAcc diag_zero() {
    return DiagAcc{0.0, 0.0, 0.0, 0.0, 0.0, -__builtin_inf(), 0.0, 0.0, 0.0, 0.0, 0.0};
}

// a <- a merged with b (a's samples first). An empty side leaves the other unchanged, bit for bit.
__device__ __forceinline__ void diag_merge(DiagAcc& a, const DiagAcc& b) {
    a.kl += b.kl;
    a.rsum += b.rsum;
    a.clip += b.clip;
    a.vclip += b.vclip;
    a.nonfin += b.nonfin;
    if (b.rmax > a.rmax) a.rmax = b.rmax;
    if (b.cnt == 0.0) return;
    if (a.cnt == 0.0) {
        a.cnt = b.cnt; a.mx = b.mx; a.m2x = b.m2x; a.my = b.my; a.m2y = b.m2y;
        return;
    }
    const double n = a.cnt + b.cnt, wb = b.cnt / n, wab = a.cnt * b.cnt / n;
    const double dx = b.mx - a.mx, dy = b.my - a.my;
    a.mx = a.mx + dx * wb;
    a.m2x = (a.m2x + b.m2x) + dx * dx * wab;
    a.my = a.my + dy * wb;
    a.m2y = (a.m2y + b.m2y) + dy * dy * wab;
    a.cnt = n;
}

__device__ __forceinline__ DiagAcc diag_shfl_down(const DiagAcc& a, int o) {
    DiagAcc b;
    b.kl = __shfl_down(a.kl, o); b.rsum = __shfl_down(a.rsum, o); b.clip = __shfl_down(a.clip, o);
    b.vclip = __shfl_down(a.vclip, o); b.nonfin = __shfl_down(a.nonfin, o); b.rmax = __shfl_down(a.rmax, o);
    b.cnt = __shfl_down(a.cnt, o); b.mx = __shfl_down(a.mx, o); b.m2x = __shfl_down(a.m2x, o);
    b.my = __shfl_down(a.my, o); b.m2y = __shfl_down(a.m2y, o);
    return b;
}

__device__ __forceinline__ void diag_store(double* p, const DiagAcc& a) {
    p[kPKl] = a.kl; p[kPRsum] = a.rsum; p[kPClip] = a.clip; p[kPVclip] = a.vclip; p[kPNonfin] = a.nonfin;
    p[kPRmax] = a.rmax; p[kPCnt] = a.cnt; p[kPMeanX] = a.mx; p[kPM2X] = a.m2x; p[kPMeanY] = a.my;
    p[kPM2Y] = a.m2y; p[kPPad] = 0.0;
}
__device__ __forceinline__ DiagAcc diag_load(const double* p) {
    return DiagAcc{p[kPKl], p[kPRsum], p[kPClip], p[kPVclip], p[kPNonfin], p[kPRmax],
                   p[kPCnt], p[kPMeanX], p[kPM2X], p[kPMeanY], p[kPM2Y]};
}
}  // namespace

// Block b takes samples b * 256 + tid, then strides by the grid: each thread folds its samples in index
// order (Welford for the two variances), the wave merges its lanes as a shuffle tree, thread 0 the
// block's waves in order. One partial per block.
__global__ __launch_bounds__(kDiagBlock) void k_diag_partials(const float* __restrict__ old_logp,
                                                              const float* __restrict__ new_logp,
                                                              const float* __restrict__ old_value,
                                                              const float* __restrict__ new_value,
                                                              const float* __restrict__ returns, long long n,
                                                              double eps, double* __restrict__ partials) {
    __shared__ double sw[kDiagWaves][kDiagSlots];
    DiagAcc a = diag_zero();
    const long long stride = (long long)gridDim.x * kDiagBlock;
    for (long long i = (long long)blockIdx.x * kDiagBlock + threadIdx.x; i < n; i += stride) {
        const double d = (double)new_logp[i] - (double)old_logp[i];
        const double r = exp(d);
        const double ov = (double)old_value[i], R = (double)returns[i];
        a.kl += (r - 1.0) - d;
        a.rsum += r;
        if (fabs(r - 1.0) > eps) a.clip += 1.0;
        if (fabs((double)new_value[i] - ov) > eps) a.vclip += 1.0;
        if (!__builtin_isfinite(d)) a.nonfin += 1.0;
        if (r > a.rmax) a.rmax = r;
        a.cnt += 1.0;
        const double x = R - ov, dx = x - a.mx, dy = R - a.my;
        a.mx += dx / a.cnt;
        a.m2x += dx * (x - a.mx);
        a.my += dy / a.cnt;
        a.m2y += dy * (R - a.my);
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const DiagAcc b = diag_shfl_down(a, o);
        diag_merge(a, b);  // lane 0's tree only reads lanes inside the wave
    }
    const int w = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) diag_store(sw[w], a);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kDiagWaves; ++k) diag_merge(a, diag_load(sw[k]));
        diag_store(partials + (size_t)blockIdx.x * kDiagSlots, a);
    }
}

// One block: the np <= kDiagMaxBlocks partials staged in LDS by all threads (one round of loads),
// merged by thread 0 in index order, then the outputs.
__global__ __launch_bounds__(kDiagBlock) void k_diag_finish(const double* __restrict__ partials, int np,
                                                            double* __restrict__ out) {
    __shared__ double sp[kDiagMaxBlocks * kDiagSlots];
    for (int i = threadIdx.x; i < np * kDiagSlots; i += kDiagBlock) sp[i] = partials[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    DiagAcc a = diag_load(sp);
    for (int k = 1; k < np; ++k) diag_merge(a, diag_load(sp + k * kDiagSlots));
    const double var_x = a.m2x / a.cnt, var_y = a.m2y / a.cnt;
    out[UAVHIP_DIAG_APPROX_KL] = a.kl / a.cnt;
    out[UAVHIP_DIAG_CLIP_FRAC] = a.clip / a.cnt;
    out[UAVHIP_DIAG_RATIO_MAX] = a.rmax;
    out[UAVHIP_DIAG_RATIO_MEAN] = a.rsum / a.cnt;
    out[UAVHIP_DIAG_VALUE_CLIP_FRAC] = a.vclip / a.cnt;
    // constant returns: NaN, the stable-baselines convention (explained_variance of a constant target)
    out[UAVHIP_DIAG_EXPLAINED_VAR] = var_y == 0.0 ? __builtin_nan("") : 1.0 - var_x / var_y;
    out[UAVHIP_DIAG_NONFINITE] = a.nonfin;
    out[UAVHIP_DIAG_RETURN_VAR] = var_y;
    out[UAVHIP_DIAG_RESIDUAL_VAR] = var_x;
}

}  // namespace uavhip

using namespace uavhip;

static int diag_blocks(int64_t n) {
    const int64_t b = (n + kDiagBlock - 1) / kDiagBlock;
    return (int)(b < kDiagMaxBlocks ? b : kDiagMaxBlocks);
}

extern "C" int32_t uavhip_ppo_diagnostics_partials(int64_t n) { return n >= 1 ? diag_blocks(n) * kDiagSlots : -1; }

extern "C" int uavhip_ppo_diagnostics(const float* old_logp, const float* new_logp, const float* old_value,
                                      const float* new_value, const float* returns, int64_t n, double eps_clip,
                                      double* partials, int32_t partials_doubles, double* out,
                                      uavhip_stream_t stream) {
    if (n < 1) {
        set_error("uavhip_ppo_diagnostics: n=%lld must be >= 1", (long long)n);
        return UAVHIP_EINVAL;
    }
    if (!old_logp || !new_logp || !old_value || !new_value || !returns || !partials || !out) {
        set_error("uavhip_ppo_diagnostics: NULL pointer (old_logp=%p new_logp=%p old_value=%p new_value=%p returns=%p "
                  "partials=%p out=%p)", (const void*)old_logp, (const void*)new_logp, (const void*)old_value,
                  (const void*)new_value, (const void*)returns, (const void*)partials, (const void*)out);
        return UAVHIP_EINVAL;
    }
    const int np = diag_blocks(n);
    if (partials_doubles < np * kDiagSlots) {
        set_error("uavhip_ppo_diagnostics: partials holds %d doubles, n=%lld needs %d "
                  "(uavhip_ppo_diagnostics_partials)", partials_doubles, (long long)n, np * kDiagSlots);
        return UAVHIP_EINVAL;
    }
    hipLaunchKernelGGL(k_diag_partials, dim3(np), dim3(kDiagBlock), 0, (hipStream_t)stream, old_logp, new_logp,
                       old_value, new_value, returns, (long long)n, eps_clip, partials);
    if (const int rc = check_launch("k_diag_partials")) return rc;
    hipLaunchKernelGGL(k_diag_finish, dim3(1), dim3(kDiagBlock), 0, (hipStream_t)stream, (const double*)partials, np,
                       out);
    return check_launch("k_diag_finish");
}
