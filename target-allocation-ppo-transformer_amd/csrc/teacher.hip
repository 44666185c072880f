// teacher.hip -- teacher-forced episodes (uavhip_teacher_steps): walk every env along a GIVEN
// allocation and record what a policy would have seen (the window each action was decided on) and
// should have done (the action), with the env's own rewards. The trace that realises an allocation
// depends on the env -- an assign is accepted only if r(X') >= r(X), and the pointer walk goes on
// differently after a rejection -- so the action is derived in the kernel, from the pointer:
//     a = (teach[u] == t) ? 1 : 0
// with teach[u] the list index of UAV u's target (lane u) and (u, t) the env's pointer. A rejected
// assign walks on (t + 1): the UAV's teacher index is behind the pointer from then on, so it stays
// unassigned for the rest of the episode. Built with -ffp-contract=off: the step is step_once
// (env_device.hpp) in an instantiation of its own, bitwise the step uavhip_env_step replays.
//
// k_env_step's shape: one wave per env, four per workgroup, the env state in registers across the
// launch, pair probabilities read from global memory (no LDS table; the only LDS is push_obs' 16-float
// row scratch per wave). Episodes end anywhere between N and N * M steps: a finished env is held
// (UAVHIP_STEP_HOLD), its rows are a zero window, action -1, reward 0, done 1.
#include "env_device.hpp"

#pragma clang fp contract(off)

namespace uavhip {
using namespace envdev;
namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kBlock = kWavesPerBlock * kWave;
constexpr int kTeacherTag = 1;  // step_once TAG: this kernel's own HOLD instantiation

template <int TPL>
__global__ __launch_bounds__(kBlock) void k_teacher_steps(uavhip_env env, const int* __restrict__ assignment, int n_max,
                                                          float* __restrict__ obs_out, int8_t* __restrict__ act_out,
                                                          double* __restrict__ reward_out,
                                                          uint8_t* __restrict__ done_out, double* __restrict__ info_out,
                                                          int* __restrict__ steps, uint8_t* __restrict__ finished,
                                                          double* __restrict__ ep_return, int* __restrict__ stats) {
    __shared__ __attribute__((aligned(16))) float s_row[kWavesPerBlock * 16];
    const int lane = lane_id();
    const int e = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (e >= env.E) return;
    const int N = env.N, M = env.M;
    EnvRegs<TPL> R;
    R.tab = nullptr;
    R.row = s_row + (threadIdx.x >> 6) * 16;
    load_regs<TPL>(R, env, e, lane);

    // target ids -> list indices of the active scene, as k_refine: a ballot against the lanes' ids,
    // the lowest list index of a duplicated id; an id that matches nothing counts as -1
    int teach = -1, invalid = 0;
    {
        int id[TPL];
#pragma unroll
        for (int j = 0; j < TPL; ++j) {
            const int t = lane + kWave * j;
            id[j] = t < M ? env.tgt_id[R.sb * M + t] : 0;
        }
        const int idin = lane < N ? assignment[(long long)e * N + lane] : -1;
        for (int u = 0; u < N; ++u) {
            const int want = readlane_i(idin, u);
            if (want == -1) continue;
            int idx = -1;
#pragma unroll
            for (int j = TPL - 1; j >= 0; --j) {
                const unsigned long long m = ballot(lane + kWave * j < M && id[j] == want);
                if (m) idx = kWave * j + ffs64(m);
            }
            if (idx < 0) ++invalid;
            if (lane == u) teach = idx;
        }
    }

    const long long E = env.E;
    if (obs_out) {  // the window step 0 is decided on: the env's own, or zeros for an env held from step 0
        const bool fin = R.u >= N;
        write_obs(obs_out + (long long)e * kObs, fin ? 0.0f : R.w0, fin ? 0.0f : R.w1, lane, false);
    }
    int cnt = 0, rejected = 0;
    double ret = ep_return ? ep_return[e] : 0.0;
    for (int t = 0; t < n_max; ++t) {
        const long long se = (long long)t * E + e;
        const bool was = R.u >= N;
        const int a = (!was && readlane_i(teach, R.u) == R.t) ? 1 : 0;
        const int nasg = R.nasg;
        // the step's reward comes back through a local: lane 0 holds it (step_once writes from lane 0)
        double rew = 0.0;
        step_once<TPL, false, true, kTeacherTag>(R, env, e, lane, a, UAVHIP_STEP_HOLD,
                                                 (obs_out && t + 1 < n_max) ? obs_out + (se + E) * kObs : nullptr, &rew,
                                                 done_out ? done_out + se : nullptr,
                                                 info_out ? info_out + se * UAVHIP_INFO_COUNT : nullptr);
        rew = readlane_d(rew, 0);
        if (!was) {
            ++cnt;
            ret = ret + rew;
            if (a == 1 && R.nasg == nasg) ++rejected;  // reward 0, nothing but the pointer moved
        }
        if (lane == 0) {
            if (reward_out) reward_out[se] = rew;
            if (act_out) act_out[se] = was ? (int8_t)-1 : (int8_t)a;
        }
    }
    store_regs(R, env, e, lane);
    if (lane == 0) {
        steps[e] += cnt;
        finished[e] = R.u >= N ? 1 : 0;
        if (ep_return) ep_return[e] = ret;
        if (stats) {
            stats[(long long)e * 2] = rejected;
            stats[(long long)e * 2 + 1] = invalid;
        }
    }
}

}  // namespace
}  // namespace uavhip

extern "C" int uavhip_teacher_steps(const uavhip_env* env, const int32_t* assignment, int32_t n_max, float* obs,
                                    int8_t* actions, double* reward, uint8_t* done, double* info, int32_t* steps,
                                    uint8_t* finished, double* ep_return, int32_t* stats, uavhip_stream_t stream) {
    using namespace uavhip;
    if (const int rc = validate_env_for("uavhip_teacher_steps", env, true)) return rc;
    if (n_max < 1 || !assignment || !steps || !finished) {
        set_error("uavhip_teacher_steps: need n_max=%d >= 1 and assignment/steps/finished non-NULL", n_max);
        return UAVHIP_EINVAL;
    }
    if (const int rc = require_f32_obs("uavhip_teacher_steps", env)) return rc;
    UAVHIP_WAVE_LAUNCH(env, k_teacher_steps<TPL>, 0, stream, *env, assignment, (int)n_max, obs, actions, reward, done, info,
                       steps, finished, ep_return, stats);
    return check_launch("k_teacher_steps");
}
