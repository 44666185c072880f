// metrics.hip -- per-episode training statistics of main_train.py:122-136 (the sums behind its CSV
// columns, :161-195) accumulated on device over rollout chunks: one thread per env walks the
// chunk in time order, so no per-step host sync is needed to log training curves.
#include "common.hpp"

namespace uavhip {

__global__ __launch_bounds__(256) void k_episode_stats(const double* __restrict__ reward,
                                                       const uint8_t* __restrict__ done,
                                                       const int8_t* __restrict__ action,
                                                       const double* __restrict__ info,
                                                       const float* __restrict__ value, int T, int E,
                                                       double* __restrict__ acc, double* __restrict__ records,
                                                       int max_records, uint32_t* __restrict__ n_records) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    double a[UAVHIP_EP_COUNT];
    double* ae = acc + (size_t)e * UAVHIP_EP_COUNT;
#pragma unroll
    for (int i = 0; i < UAVHIP_EP_COUNT; ++i) a[i] = ae[i];
    for (int t = 0; t < T; ++t) {
        const size_t te = (size_t)t * E + e;
        if (a[UAVHIP_EP_STEPS] == 0.0) a[UAVHIP_EP_Q0] = (double)value[te];  // episode start state
        const double* in = info + te * UAVHIP_INFO_COUNT;
        const double ncov = in[UAVHIP_INFO_NUM_ASSIGNED];
        a[UAVHIP_EP_STEPS] += 1.0;
        a[UAVHIP_EP_REWARD] = a[UAVHIP_EP_REWARD] + reward[te];
        a[UAVHIP_EP_J_SUM] = a[UAVHIP_EP_J_SUM] + in[UAVHIP_INFO_J];
        a[UAVHIP_EP_MAX_COV] = ncov > a[UAVHIP_EP_MAX_COV] ? ncov : a[UAVHIP_EP_MAX_COV];
        if (action[te] == 1) {
            a[UAVHIP_EP_ACTION1] += 1.0;
            if (in[UAVHIP_INFO_IS_VALID] == 1.0) a[UAVHIP_EP_VALID] += 1.0;
        }
        if (ncov > 0.0) {
            a[UAVHIP_EP_PDMG_SUM] = a[UAVHIP_EP_PDMG_SUM] + in[UAVHIP_INFO_AVG_P_DMG];
            a[UAVHIP_EP_PFINAL_SUM] = a[UAVHIP_EP_PFINAL_SUM] + in[UAVHIP_INFO_AVG_P_FINAL];
            a[UAVHIP_EP_ASSIGN_STEPS] += 1.0;
        }
        if (done[te]) {
            a[UAVHIP_EP_ENV] = (double)e;
            a[UAVHIP_EP_EPISODE] = in[UAVHIP_INFO_EPISODE];
            const uint32_t slot = atomicAdd(n_records, 1u);
            if ((int)slot < max_records) {
                double* r = records + (size_t)slot * UAVHIP_EP_COUNT;
#pragma unroll
                for (int i = 0; i < UAVHIP_EP_COUNT; ++i) r[i] = a[i];
            }
#pragma unroll
            for (int i = 0; i < UAVHIP_EP_COUNT; ++i) a[i] = 0.0;
        }
    }
#pragma unroll
    for (int i = 0; i < UAVHIP_EP_COUNT; ++i) ae[i] = a[i];
}

// Best of K (uavhip_select_best): one wave per scene. Every lane walks the scene's K replicas
// (e = s * K + k; wave-uniform loads) for the finished one with the largest J, the lowest k on a tie;
// lane u then writes UAV u's target id of that replica.
__global__ __launch_bounds__(256) void k_select_best(uavhip_env env, int K, int S, int* __restrict__ best,
                                                     double* __restrict__ J, int* __restrict__ covered,
                                                     int* __restrict__ assignment) {
    const int s = blockIdx.x * (blockDim.x / kWave) + (threadIdx.x >> 6), lane = threadIdx.x & (kWave - 1);
    if (s >= S) return;
    int kb = -1;
    double jb = 0.0;
    for (int k = 0; k < K; ++k) {
        const long long e = (long long)s * K + k;
        if (env.istate[e * UAVHIP_IST_COUNT + UAVHIP_IST_UAV_IDX] < env.N) continue;  // not finished
        const double j = env.dstate[e * UAVHIP_DST_COUNT + UAVHIP_DST_J];
        if (kb < 0 || j > jb) {
            kb = k;
            jb = j;
        }
    }
    const long long e = (long long)s * K + (kb < 0 ? 0 : kb);
    const int* is = env.istate + e * UAVHIP_IST_COUNT;
    if (lane == 0) {
        best[s] = kb;
        J[s] = jb;
        covered[s] = kb < 0 ? 0 : is[UAVHIP_IST_N_COVERED];
    }
    for (int u = lane; u < env.N; u += kWave) {
        int id = -1;
        if (kb >= 0) {
            const int t = env.assigned[e * env.N + u];
            const long long sb = (env.scene_buffers == 2 ? (long long)(is[UAVHIP_IST_SCENE_SEL] & 1) * env.E : 0) + e;
            if (t >= 0) id = env.tgt_id[sb * env.M + t];
        }
        assignment[(long long)s * env.N + u] = id;
    }
}

}  // namespace uavhip

extern "C" int uavhip_select_best(const uavhip_env* env, int32_t K, int32_t* best, double* J, int32_t* covered,
                                  int32_t* assignment, uavhip_stream_t stream) {
    using namespace uavhip;
    if (const int rc = validate_env(env, true)) return rc;
    if (K <= 0 || env->E % K != 0 || !best || !J || !covered || !assignment) {
        set_error("uavhip_select_best: K=%d must be > 0 and divide E=%d, and best/J/covered/assignment non-NULL", K,
                  env->E);
        return UAVHIP_EINVAL;
    }
    const int S = env->E / K;
    hipLaunchKernelGGL(k_select_best, dim3((S + 3) / 4), dim3(256), 0, (hipStream_t)stream, *env, (int)K, S, best, J,
                       covered, assignment);
    return check_launch("k_select_best");
}

extern "C" int uavhip_episode_stats(const double* reward, const uint8_t* done, const int8_t* action,
                                    const double* info, const float* value, int32_t T, int32_t E, double* acc,
                                    double* records, int32_t max_records, uint32_t* n_records,
                                    uavhip_stream_t stream) {
    using namespace uavhip;
    if (!reward || !done || !action || !info || !value || !acc || !n_records || (max_records > 0 && !records) ||
        T <= 0 || E <= 0 || max_records < 0) {
        set_error("uavhip_episode_stats: NULL pointer or bad sizes (T=%d, E=%d, max_records=%d)", T, E, max_records);
        return UAVHIP_EINVAL;
    }
    hipLaunchKernelGGL(k_episode_stats, dim3((E + 255) / 256), dim3(256), 0, (hipStream_t)stream, reward, done, action,
                       info, value, (int)T, (int)E, acc, records, (int)max_records, n_records);
    return check_launch("k_episode_stats");
}
