// policy_steps.hpp -- the argument structs and launchers of the multi-step kernels: the only interface
// between policy.hip (the C entry points, which call the launchers) and rollout_steps.hip (the kernels and
// the launchers' definitions). Included by both.
#pragma once
#include "policy_block.hpp"

namespace uavhip {
namespace pol {

// Multi-step fused rollout (uavhip_rollout_steps). A workgroup's 16 envs and their windows, ring
// rows and env state are touched by no other workgroup, so one launch runs n consecutive steps of
// them with only a workgroup barrier in between (the step's global stores -- next windows, ring
// row, env state -- are read by the next step's waves of the same workgroup: __syncthreads orders
// them, workgroup scope). Step t: windows obs[t] -> actions / logp / value [t], obs[t + 1],
// reward / done / info [t]; ring step g + t; sampling counters offset + t * off_stride + b. Saves
// the per-launch tail (the slowest of 256 workgroups, +2.6 % over the median) and start-up.
struct StepSeq {
    int n;                 // steps in this launch
    long long obs_stride;  // floats from obs[t] to obs[t + 1] (E * 5 * 14)
    uint64_t off_stride;   // sampling counter advance per step
};
// All of the launch's arguments in one struct: the kernel's only parameter, so the kernarg
// segment holds exactly this struct at offset 0.
struct StepsArgs {
    const float* P;
    const float* states;
    int B;
    uint64_t seed, offset;
    const uint64_t* offset_dev;
    int8_t* action_out;
    float *logp_out, *value_out;
    RowIO rio;
    uavhip_env env;
    EnvOut eo;
    StepSeq seq;
};
// k_rollout_steps is compiled in its own translation unit (rollout_steps.hip: the same forward headers
// with UAVHIP_STEPS_TU + UAVHIP_TID_LAUNDER); uavhip_rollout_steps launches it through this.
int launch_rollout_steps(const StepsArgs& sa, hipStream_t stream);
// k_decode_steps' only parameter (uavhip_decode_steps; the same translation unit as k_rollout_steps)
struct DecodeArgs {
    const float* P;
    float* obs2;  // [2][B][5][14]: step rio.g + t reads slot (rio.g + t) & 1 and writes the other
    int B;
    uint64_t seed, offset;
    const uint64_t* offset_dev;
    RowIO rio;
    uavhip_env env;
    int n_max, greedy_stride;
    long long obs_stride;  // floats between the two slots (B * 5 * 14)
    uint64_t off_stride;   // sampling counter advance per step
    int8_t* actions;       // [n_max][B] (nullable)
    int32_t* steps;        // [B]
    uint8_t* finished;     // [B]; the env step's done flag of every step
    double* ep_return;     // [B] (nullable); between the steps the env step's reward
};
int launch_decode_steps(const DecodeArgs& da, hipStream_t stream);
// k_rollout_actor_steps (uavhip_rollout_actor_steps): k_rollout_steps' arguments, value_out not read
int launch_rollout_actor_steps(const StepsArgs& sa, hipStream_t stream);
// k_value_steps' only parameter (uavhip_value_steps; the same translation unit as k_rollout_steps)
struct ValueArgs {
    const float* P;
    const float* obs;      // [n + 1][B][5][14]: the recorded windows of one deque sequence
    int B, n;              // windows per step; steps with a value row
    long long obs_stride;  // floats from obs[t] to obs[t + 1]
    RowIO rio;             // ring step of obs[0]
    float* values;         // [n][B]
    float* last_values;    // [B]: V of obs[n] (nullable: the pass stops at obs[n - 1])
    float* stash;          // [ceil(B / 16)][5][2 * 16 * 136]: the groups' attention outputs and residual rows
};
int launch_value_steps(const ValueArgs& va, hipStream_t stream);
constexpr int kVG = S;  // k_value_steps: windows per group, one 16-token tile each

}  // namespace pol
}  // namespace uavhip
