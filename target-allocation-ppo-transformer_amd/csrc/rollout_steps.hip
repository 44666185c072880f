// rollout_steps.hip -- k_rollout_steps (uavhip_rollout_steps): policy.hip's fused rollout step in a
// loop over the steps of one launch, compiled in a translation unit of its own so that every
// lane-index expression can be laundered per use (UAVHIP_TID_LAUNDER, common.hpp tid_x()) without
// touching the code of the single-step kernels. k_decode_steps (uavhip_decode_steps), the actor-only
// inference loop, lives here for the same reason, and so do k_rollout_actor_steps / k_value_steps
// (uavhip_rollout_actor_steps, uavhip_value_steps), the rollout with the critic off the step chain.
#define UAVHIP_STEPS_TU 1
#define UAVHIP_TID_LAUNDER 1
#include "policy.hip"
