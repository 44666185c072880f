// expert.hip -- on-policy expert labels (uavhip_expert_steps): walk every env along an ARBITRARY
// action trace (a learner's own, or the expert's) and record, per step, the window the action was
// decided on, the action taken, and what the state-wise expert would have done in that state:
//     label = 1 iff g[t] > 0.0 and g[t'] <= g[t] for every t < t' < M
// at the pointer (u, t), with g[t'] UAV u's marginal gain on target t' against the current locks
// (include/uavhip.h has the rule with its order of operations). That is DAgger's relabelling step.
// Following the labels from a reset is one best-response sweep from the empty assignment
// (uavhip_refine_assignments(NULL, max_sweeps = 1)).
//
// k_teacher_steps' shape: one wave per env, four per workgroup, the env state in registers across
// the launch, a finished env held (UAVHIP_STEP_HOLD), the step step_once (env_device.hpp) in an
// instantiation of its own. Built with -ffp-contract=off.
//
// Q[t'] is the env's own running product nh_final[t'] (EnvRegs::nhf): step_once multiplies
// (1.0 - pd * pp) into it at every accepted assign, from 1.0, and the walk visits the UAVs in
// ascending order with at most one assign each, so it IS the ascending-w product, bit for bit.
// While the pointer walks one UAV's targets the lock set changes only on the assign that ends the
// visit: g[] (one coalesced row of p_dmg[u][:]) and its exclusive suffix maximum (a reverse wave
// scan) are formed once per visit and the step reads two lanes of them.
#include "env_device.hpp"

#pragma clang fp contract(off)

namespace uavhip {
using namespace envdev;
namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kBlock = kWavesPerBlock * kWave;
constexpr int kExpertTag = 2;  // step_once TAG: this kernel's own HOLD instantiation

// max of x over the lanes above this one (exclusive reverse scan); -inf on lane 63. `all` gets the
// maximum over the whole wave. max is exact: the order of the scan does not show in the result.
__device__ __forceinline__ double suffix_max_excl(double x, int lane, double& all) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const double y = __shfl_down(x, d);
        if (lane + d < kWave) x = y > x ? y : x;
    }
    all = readlane_d(x, 0);
    const double up = __shfl_down(x, 1);
    return lane < kWave - 1 ? up : -__builtin_huge_val();
}

template <int TPL>
__global__ __launch_bounds__(kBlock) void k_expert_steps(uavhip_env env, const int8_t* __restrict__ actions_in,
                                                         const uint8_t* __restrict__ follow, int n_max,
                                                         float* __restrict__ obs_out, int8_t* __restrict__ act_out,
                                                         int8_t* __restrict__ label_out, double* __restrict__ margin_out,
                                                         double* __restrict__ reward_out, uint8_t* __restrict__ done_out,
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

    const bool follows = !actions_in || (follow && readlane_i((int)follow[e], 0) != 0);
    const double omega = env.prm[UAVHIP_PRM_OMEGA];
    const double ninf = -__builtin_huge_val();
    const long long E = env.E;

    double g[TPL], sm[TPL];  // g[t'] of the visited UAV and max_{t'' > t'} g[t''] (-inf: none)
#pragma unroll
    for (int k = 0; k < TPL; ++k) g[k] = sm[k] = ninf;
    int gu = -1;             // the UAV g[] / sm[] were formed for
    int cnt = 0, rejected = 0, differ = 0, ended = 0;
    double ret = ep_return ? ep_return[e] : 0.0;
    for (int t = 0; t < n_max; ++t) {
        const long long se = (long long)t * E + e;
        bool live = R.u < N && !ended;
        int a = 0, label = 0;
        double margin = 0.0;
        if (live) {
            const int u = R.u;
            if (u != gu) {  // a new visit: the locks changed (or the launch starts here)
                const double pu = readlane_d(R.ppen, u);
                const double wcu = omega * readlane_d(R.ucost, u);
                const double* __restrict__ prow = env.p_dmg + (R.sb * N + u) * M;
#pragma unroll
                for (int k = 0; k < TPL; ++k) {
                    const int tt = lane + kWave * k;
                    g[k] = ninf;
                    if (tt < M) {
                        const double p = prow[tt] * pu;
                        g[k] = (R.val[k] * R.nhf[k]) * p - wcu;
                    }
                }
                double above = ninf;  // the maximum over the slots above slot k
#pragma unroll
                for (int k = TPL - 1; k >= 0; --k) {
                    double all;
                    const double s = suffix_max_excl(g[k], lane, all);
                    sm[k] = s > above ? s : above;
                    above = all > above ? all : above;
                }
                gu = u;
            }
            const int tl = R.t & 63, tk = R.t >> 6;
            const double gt = pick(g, tk, tl), later = pick(sm, tk, tl);
            label = (gt > 0.0 && later <= gt) ? 1 : 0;
            margin = gt - (later > 0.0 ? later : 0.0);
            a = follows ? label : readlane_i((int)actions_in[se], 0);
            if (a != 0 && a != 1) {  // the trace ends here: the env is held, live, for the rest of the call
                ended = 1;
                live = false;
            }
        }
        // the window this step's action is decided on; a held row's is zero
        if (obs_out) write_obs(obs_out + se * kObs, live ? R.w0 : 0.0f, live ? R.w1 : 0.0f, lane, false);
        double rew = 0.0;
        if (live) {
            const int nasg = R.nasg;
            // the step's reward comes back through a local: lane 0 holds it (step_once writes from lane 0)
            step_once<TPL, false, true, kExpertTag>(R, env, e, lane, a, UAVHIP_STEP_HOLD, nullptr, &rew,
                                                    done_out ? done_out + se : nullptr, nullptr);
            rew = readlane_d(rew, 0);
            ++cnt;
            ret = ret + rew;
            if (a == 1 && R.nasg == nasg) ++rejected;  // reward 0, nothing but the pointer moved
            if (a != label) ++differ;
        } else if (done_out && lane == 0) {
            done_out[se] = 1;
        }
        if (lane == 0) {
            if (reward_out) reward_out[se] = rew;
            if (act_out) act_out[se] = live ? (int8_t)a : (int8_t)-1;
            if (label_out) label_out[se] = live ? (int8_t)label : (int8_t)-1;
            if (margin_out) margin_out[se] = live ? margin : 0.0;
        }
    }
    store_regs(R, env, e, lane);
    if (lane == 0) {
        steps[e] += cnt;
        finished[e] = R.u >= N ? 1 : 0;
        if (ep_return) ep_return[e] = ret;
        if (stats) {
            stats[(long long)e * 3] = rejected;
            stats[(long long)e * 3 + 1] = differ;
            stats[(long long)e * 3 + 2] = ended;
        }
    }
}

}  // namespace
}  // namespace uavhip

extern "C" int uavhip_expert_steps(const uavhip_env* env, const int8_t* actions_in, const uint8_t* follow,
                                   int32_t n_max, float* obs, int8_t* actions, int8_t* labels, double* margin,
                                   double* reward, uint8_t* done, int32_t* steps, uint8_t* finished, double* ep_return,
                                   int32_t* stats, uavhip_stream_t stream) {
    using namespace uavhip;
    if (const int rc = validate_env_for("uavhip_expert_steps", env, true)) return rc;
    if (n_max < 1 || !steps || !finished) {
        set_error("uavhip_expert_steps: need n_max=%d >= 1 and steps/finished non-NULL", n_max);
        return UAVHIP_EINVAL;
    }
    if (follow && !actions_in) {
        set_error("uavhip_expert_steps: follow needs actions_in (without a trace every env follows the expert)");
        return UAVHIP_EINVAL;
    }
    if (const int rc = require_f32_obs("uavhip_expert_steps", env)) return rc;
    UAVHIP_WAVE_LAUNCH(env, k_expert_steps<TPL>, 0, stream, *env, actions_in, follow, (int)n_max, obs, actions, labels,
                       margin, reward, done, steps, finished, ep_return, stats);
    return check_launch("k_expert_steps");
}
