/*
 * uavhip.h -- C ABI of libuavhip.so, the MI355X (gfx950) implementation of the PPO rollout
 * hot path of the UAV->target allocation reference (envs/uav_env.py, envs/mechanics.py,
 * networks/transformer_net.py, agents/ppo.py).
 *
 * The reference has no FFI layer: its boundary is the Python object API that main_train.py
 * calls (UAVEnv.reset/step, PPOAgent.select_action/store_transition/update). Each entry point
 * below replaces one piece of that API; the Python mirror in
 * target-allocation-ppo-transformer_amd/uavhip binds them with ctypes.
 *
 * Conventions
 *  - every pointer is CALLER-OWNED DEVICE memory (torch tensors), except the `const
 *    uavhip_env*` / `const uavhip_policy*` descriptors themselves, which live on the host and are
 *    copied into the launch; the library never allocates or frees on the hot path;
 *  - every call is asynchronous on `stream` (a hipStream_t; NULL = the legacy default stream)
 *    and never synchronises the device;
 *  - return 0 on success, a negative UAVHIP_E* code otherwise; uavhip_last_error() returns a
 *    thread-local message. No C++ exception crosses this boundary;
 *  - layouts are row-major, env index outermost ("[E][N][M]" = e*N*M + u*M + t).
 */
#ifndef UAVHIP_H
#define UAVHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* uavhip_stream_t; /* hipStream_t */

#define UAVHIP_SEQ_LEN 5    /* config.py:62 SEQ_LEN    */
#define UAVHIP_STATE_DIM 14 /* config.py:61 STATE_DIM  */
#define UAVHIP_OBS_FLOATS (UAVHIP_SEQ_LEN * UAVHIP_STATE_DIM)
#define UAVHIP_MAX_N 64     /* UAVs per env (one wave lane each)          */
#define UAVHIP_MAX_M 128    /* targets per env (<= 2 per wave lane)       */
#define UAVHIP_MAX_OBSTACLES 8
/* uavhip_env.flags */
#define UAVHIP_ENV_ONE_PER_WAVE 1  /* multi-step launches: never pack two envs into one wave */
#define UAVHIP_ENV_OBS_F16 2       /* obs_out of uavhip_env_reset / uavhip_env_step is IEEE binary16
                                      (round-to-nearest-even of the f32 window; BASELINE config 4)
                                      instead of f32; the env's own window stays f32          */
#define UAVHIP_ENV_NO_REPLAY 4     /* multi-step launches: never use the omega = 0 replay kernel
                                      (K2r, env_replay.hpp), always the step-by-step K2 / K2g.
                                      K2r assumes every tentative assign is accepted, which
                                      omega = 0 guarantees only when every target value is >= 0
                                      (J can then never drop, uav_env.py:317-338; pair
                                      probabilities are clipped to [0, 1] by construction). The
                                      generators never make a negative value; a caller loading
                                      host scenes that may must set this flag (VecUAVEnv.
                                      load_scenes does it).                                      */

enum uavhip_status {
    UAVHIP_OK = 0,
    UAVHIP_EINVAL = -1, /* bad argument / shape */
    UAVHIP_EHIP = -2,   /* HIP launch or runtime error */
};

/* Physics constants (config.py:7-12,53 / config0.py), passed by value. */
enum uavhip_param {
    UAVHIP_PRM_ZETA_D = 0, /* PARAM_ZETA_D, target distance scale (150)        */
    UAVHIP_PRM_K,          /* PARAM_K, speed ratio weight (1.2; 5.0 in config0)  */
    UAVHIP_PRM_C1,         /* PARAM_C1 */
    UAVHIP_PRM_C2,         /* PARAM_C2 */
    UAVHIP_PRM_C3,         /* PARAM_C3 */
    UAVHIP_PRM_C4,         /* PARAM_C4 */
    UAVHIP_PRM_OMEGA,      /* COST_WEIGHT_OMEGA */
    UAVHIP_PRM_ZETA_OBS,   /* obstacle distance scale, 10 (mechanics.py:79)      */
    UAVHIP_PRM_COUNT
};

/* On-device scene generator ranges (uav_env.py:65-173). */
enum uavhip_gen {
    UAVHIP_GEN_UAV_X0 = 0, UAVHIP_GEN_UAV_X1, /* UAV_GEN_X_RANGE            */
    UAVHIP_GEN_TGT_X0, UAVHIP_GEN_TGT_X1,     /* TARGET_GEN_X_RANGE         */
    UAVHIP_GEN_MAP_H,                         /* MAP_HEIGHT                 */
    UAVHIP_GEN_WEATHER_SPEED,                 /* WEATHER_SPEED_FACTOR       */
    UAVHIP_GEN_WEATHER_LOAD,                  /* WEATHER_LOAD_FACTOR        */
    UAVHIP_GEN_NFZ_X0, UAVHIP_GEN_NFZ_X1,     /* 120, 140 (uav_env.py:150)  */
    UAVHIP_GEN_ICP_X0, UAVHIP_GEN_ICP_X1,     /* 140, 160 (uav_env.py:160)  */
    UAVHIP_GEN_ICP_S0, UAVHIP_GEN_ICP_S1,     /* 0.30, 0.32 (uav_env.py:164)*/
    UAVHIP_GEN_COUNT = 16
};

/* Per-step diagnostics (uav_env.py:426-433 `info`), one row of doubles per env-step. */
enum uavhip_info {
    UAVHIP_INFO_J = 0,          /* J_val after the action (_calc_J_X)               */
    UAVHIP_INFO_NUM_ASSIGNED,   /* num_assigned = N0, covered targets                */
    UAVHIP_INFO_IS_VALID,       /* is_valid_action: 1/0, or -1 for None (action 0)   */
    UAVHIP_INFO_AVG_P_DMG,      /* avg_p_dmg over locked pairs                       */
    UAVHIP_INFO_AVG_P_FINAL,    /* avg_p_final over locked pairs                     */
    UAVHIP_INFO_UAV_IDX,        /* pointer after the action (before any auto-reset)  */
    UAVHIP_INFO_TARGET_IDX,
    UAVHIP_INFO_EPISODE,        /* 1-based episode index the step belonged to        */
    UAVHIP_INFO_COUNT
};

/* Integer per-env scalars, istate[E][UAVHIP_IST_COUNT]. */
enum uavhip_ist {
    UAVHIP_IST_UAV_IDX = 0, /* uav_env.py:33 self.uav_idx    */
    UAVHIP_IST_TARGET_IDX,  /* uav_env.py:34 self.target_idx */
    UAVHIP_IST_N_COVERED,   /* N0: targets with >= 1 lock    */
    UAVHIP_IST_N_ASSIGNED,  /* locked (uav, target) pairs    */
    UAVHIP_IST_EPISODE,     /* 1-based episode counter (main_train.py:77-79 cadence) */
    UAVHIP_IST_ERROR,       /* bit 0: a finished env was stepped without auto-reset;
                               bit 1: a full reset found no fresh spare scene (state-only reset done) */
    UAVHIP_IST_SCENE_SEL,   /* active scene buffer (0/1) when scene_buffers == 2 */
    UAVHIP_IST_SCENE_STALE, /* 1: the spare buffer still holds a used scene (uavhip_scene_refresh) */
    UAVHIP_IST_SCENE_GEN,   /* number of on-device scenes generated for this env = the number of the next
                               one (Philox counter word 2; "Scene counters" at uavhip_scene_generate) */
    UAVHIP_IST_PAD0, UAVHIP_IST_PAD1, UAVHIP_IST_PAD2,
    UAVHIP_IST_COUNT
};

/* Float64 per-env scalars, dstate[E][UAVHIP_DST_COUNT]. */
enum uavhip_dst {
    UAVHIP_DST_R = 0,      /* cached r(X) (_calculate_paper_reward of the current state) */
    UAVHIP_DST_J,          /* cached J(X)                                                */
    UAVHIP_DST_ASG_COST,   /* sum of costs of unavailable UAVs (chi_c numerator)         */
    UAVHIP_DST_COV_VALUE,  /* sum of values of covered targets (chi_v numerator)         */
    UAVHIP_DST_TOTAL_COST, /* total_swarm_cost (uav_env.py:118)                          */
    UAVHIP_DST_TOTAL_VALUE,/* sum of target values                                       */
    UAVHIP_DST_PD_CUR,     /* p_dmg of the current pointer pair (cached: no dependent load) */
    UAVHIP_DST_SUM_PDMG,   /* sum of p_dmg over locked pairs, in lock order (info avg_p_dmg)     */
    UAVHIP_DST_SUM_PFIN,   /* sum of p_final over locked pairs, in lock order (info avg_p_final) */
    UAVHIP_DST_PAD0, UAVHIP_DST_PAD1, UAVHIP_DST_PAD2,
    UAVHIP_DST_COUNT
};

/*
 * Vectorised env descriptor: E independent copies of UAVEnv (envs/uav_env.py:13) in SoA device
 * tensors. Replaces the Python objects `self.uavs / self.targets / self.nfz_list /
 * self.interceptors` (records of envs/entities.py:13-61) and the pointer/lock state.
 */
typedef struct uavhip_env {
    int32_t E, N, M, Kn, Ki;
    int32_t full_reset_period; /* auto-reset: switch to a fresh scene when episode % period == 0
                                  (200 in main_train.py:79); 0 = state-only resets. Needs
                                  scene_buffers == 2.                                         */
    int32_t scene_buffers;     /* 1, or 2 = every scene array and pair table below is
                                  [2][E]...: buffer istate[SCENE_SEL] is active, the other a
                                  pre-generated spare a full reset flips to                  */
    int32_t flags;              /* UAVHIP_ENV_* bits (0 = defaults)                    */
    uint64_t seed;             /* Philox key for on-device scene generation                 */
    uint64_t env_base;         /* global index of env 0: scene counters run on env_base + e, so
                                  a rank's shard [env_base, env_base + E) draws the scenes the
                                  same envs draw in one process over the union (0 on one GPU) */
    double prm[UAVHIP_PRM_COUNT];
    double gen[UAVHIP_GEN_COUNT];
    /* scene: entities.py records as SoA */
    double* uav_pos;   /* [E][N][2]  UAV.pos                                  */
    double* uav_vel;   /* [E][N][2]  UAV.velocity                             */
    double* uav_load;  /* [E][N]     UAV.load (weather-scaled)                */
    double* uav_cost;  /* [E][N]     UAV.cost (1.0 / 1.25)                    */
    int32_t* uav_type; /* [E][N]     UAV.uav_type                             */
    double* tgt_pos;   /* [E][M][2]  Target.pos, in LIST order (post-shuffle) */
    double* tgt_vel;   /* [E][M][2]  Target.velocity                          */
    double* tgt_value; /* [E][M]     Target.value                             */
    int32_t* tgt_id;   /* [E][M]     Target.id (pre-shuffle index)            */
    double* nfz_pos;   /* [E][Kn][2] NoFlyZone.pos                            */
    double* icp_pos;   /* [E][Ki][2] Interceptor.pos                          */
    double* icp_vel;   /* [E][Ki][2] Interceptor.velocity                     */
    /* pair tables (uavhip_score_pairs output) */
    double* p_dmg;     /* [E][N][M]  calc_damage_prob (mechanics.py:93)        */
    double* p_pen;     /* [E][N]     calc_penetration_prob (mechanics.py:118) */
    /* dynamic state */
    double* nh_final;  /* [E][M] prod over lockers of (1 - p_final), lock order  */
    double* nh_pure;   /* [E][M] prod over lockers of (1 - p_dmg)               */
    double* t_cost;    /* [E][M] sum of locker costs, lock order                */
    int32_t* n_lock;   /* [E][M] number of lockers                              */
    int32_t* assigned; /* [E][N] target LIST index or -1 (id = tgt_id[..])       */
    int32_t* istate;   /* [E][UAVHIP_IST_COUNT]                                */
    double* dstate;    /* [E][UAVHIP_DST_COUNT]                                */
    float* window;     /* [E][5][14] state_buffer deque (uav_env.py:37)        */
} uavhip_env;

/* ---------------------------------------------------------------- env (K1, K2, reset, gen) */

/* K1. Dense pair tables p_dmg[E][N][M], p_pen[E][N] of the ACTIVE scene buffer from the scene
 * arrays, for the envs with mask[e] != 0 (mask NULL = all). Replaces calc_advantage's per-call recomputation
 * (mechanics.py:93-181; called ~42x per env step by uav_env.py:184-435). */
int uavhip_score_pairs(const uavhip_env* env, const uint8_t* mask, uavhip_stream_t stream);

/* Philox4x32-10 scene generation on device (distribution of uav_env.py:65-173, not its
 * MT19937 stream) into the ACTIVE buffer of masked envs (and the spare, when scene_buffers == 2),
 * followed by K1 for them; the counter is (env, istate[SCENE_GEN]).
 *
 * Scene counters. Scene number `gen` of env e is a function of (env->seed, env_base + e, gen) alone.
 * Every draw is philox4x32_10(counter = {index, (uint32_t)(env->env_base + e), (uint32_t)gen, stream},
 * key = {(uint32_t)seed, (uint32_t)(seed >> 32)}); env indices therefore alias modulo 2^32. A double in
 * [0, 1) is u01(a, b) = (((uint64_t)a << 32 | b) >> 11) * 2^-53 of two words of one block, written
 * u01(x, y) / u01(z, w) below. Streams (index = the UAV, target list position or obstacle;
 * g[X] = env->gen[UAVHIP_GEN_X]):
 *   0  UAV i:  x the type key -- UAV i is type 2 iff the rank of its key among the N keys (ties: the
 *              lower index first) is < N / 4
 *   1  UAV i:  pos = (g[UAV_X0] + (g[UAV_X1] - g[UAV_X0]) * u01(x, y), g[MAP_H] * u01(z, w))
 *   2  UAV i:  speed = (type 1 ? 0.35 + (0.50 - 0.35) * u01(x, y) : 0.75 + (0.90 - 0.75) * u01(x, y))
 *              * g[WEATHER_SPEED]; heading = (-15 + 30 * u01(z, w)) degrees; vel = (cos, sin) * speed;
 *              load = (type 1 ? 0.95 : 1.0) * g[WEATHER_LOAD]; cost = type 1 ? 1.0 : 1.25
 *   3  index 0: n2 = min(n_remain, 1 + (int)(u01(x, y) * n_remain)), n_remain = M - M / 2 - 1 (n2 = 0
 *              and nothing read when n_remain = 0)
 *   4  target t: x the id key, y the value key -- tgt_id[t] is the rank of the id key among the M keys
 *              (ties as above); with r the rank of the value key, tgt_value[t] = 4 for r < M / 2, 6 for
 *              the next n2 ranks, 8 for the next n_remain - n2, 16 for the last
 *   5  target t: pos = (g[TGT_X0] + (g[TGT_X1] - g[TGT_X0]) * u01(x, y), g[MAP_H] * u01(z, w))
 *   6  target t: vel = ((u01(x, y) - 0.5) * 0.03, (u01(z, w) - 0.5) * 0.03)
 *   7  no-fly zone k: pos from g[NFZ_X0..X1] and g[MAP_H], as stream 5
 *   8  interceptor k: pos from g[ICP_X0..X1] and g[MAP_H], as stream 5
 *   9  interceptor k: speed = g[ICP_S0] + (g[ICP_S1] - g[ICP_S0]) * u01(x, y); heading = 2 pi u01(z, w)
 *              radians; vel = (cos, sin) * speed
 * All of it in fp64 without contraction, in the order written; cos / sin are the device library's, so
 * the two velocity fields are reproducible to its accuracy (a few ulp), everything else bit for bit
 * (tests/device_rng.py restates it; tests/test_gpu_device_rng.py compares).
 *
 * istate[SCENE_GEN] is the number of the NEXT scene to draw for the env. This call draws scene
 * SCENE_GEN into the active buffer and adds 1; with scene_buffers == 2 it then draws the following
 * number into the spare and adds 1 again. uavhip_scene_refresh draws scene SCENE_GEN into a stale spare
 * and adds 1; a full reset's flip draws nothing. So, from zeroed istate and with a refresh between any
 * two flips, the active buffer holds scene k after the env's k-th flip, the fresh spare scene k + 1, and
 * SCENE_GEN is k + 2 (k + 1 while the spare is stale). With one buffer the j-th call on an env draws
 * scene j - 1 and leaves SCENE_GEN = j. */
int uavhip_scene_generate(const uavhip_env* env, const uint8_t* mask, uavhip_stream_t stream);

/* Regenerate (Philox + K1) the spare scene buffer of every env whose istate[SCENE_STALE] is set,
 * i.e. that flipped to its spare at a full reset. Call once per rollout iteration (full resets
 * are >= full_reset_period episodes apart). No-op unless scene_buffers == 2. */
int uavhip_scene_refresh(const uavhip_env* env, uavhip_stream_t stream);

/* UAVEnv.reset(full_reset=False) (uav_env.py:42-63,175-182) for masked envs: clears the
 * allocation, recomputes the scene totals, writes the first window to obs_out[E][5][14]
 * (nullable). episode >= 0 sets istate[EPISODE]; < 0 leaves it. */
int uavhip_env_reset(const uavhip_env* env, const uint8_t* mask, int32_t episode, float* obs_out,
                     uavhip_stream_t stream);

/* K2. UAVEnv.step (uav_env.py:295-435) for all E envs, T consecutive steps fused in one launch
 * (T = 1 for the per-step rollout). actions: int8 [T][E] (0 skip, 1 assign). Outputs (each
 * nullable): obs_out [T][E][5][14] f32, reward [T][E] f64, done [T][E] u8,
 * info [T][E][UAVHIP_INFO_COUNT] f64.
 * auto_reset != 0: a finished env is reset in-kernel (state-only, or a fresh on-device scene
 * every full_reset_period episodes) and obs_out carries the NEW episode's first window;
 * auto_reset == 0: obs_out is all zeros for a finished env (the reference returns zeros(14),
 * uav_env.py:188-189) and stepping it again only sets istate[ERROR].
 * The device env step (step_once / gstep) has a third auto_reset value, UAVHIP_STEP_HOLD: as 0, but
 * a finished env is HELD -- stepping it again is not an error (istate[ERROR] is not set), its state
 * keeps every value, and the step reports a zero window, reward 0, done 1. It is compiled into the
 * decode kernel only (uavhip_decode_steps, which always runs with it: episodes of different lengths
 * in one launch); this entry point takes it as any other nonzero value. */
#define UAVHIP_STEP_HOLD 2
int uavhip_env_step(const uavhip_env* env, const int8_t* actions, int32_t T, int32_t auto_reset,
                    float* obs_out, double* reward, uint8_t* done, double* info, uavhip_stream_t stream);

/* ---------------------------------------------------------------- PPO reductions (K3) */

/* GAE over a time-major [T][E] buffer (agents/ppo.py:70-91, fp32 arithmetic in the reference's
 * op order): next_v = v[t+1] (t < T-1) or last_value[e] (NULL -> 0, the reference's value at
 * an episode end); done zeroes the bootstrap and the carry. Writes returns and raw advantages
 * (returns - values), and per-block (sum, sum of squares) partials of the advantages to
 * partials[2 * uavhip_gae_partials(T, E)] (nullable) for uavhip_adv_normalize. */
int uavhip_gae(const double* reward, const uint8_t* done, const float* value, const float* last_value,
               int32_t T, int32_t E, double gamma, double lam, float* ret, float* adv, double* partials,
               uavhip_stream_t stream);
int32_t uavhip_gae_partials(int32_t T, int32_t E);

/* fp64 (sum, sum of squares) partials of adv[n] into partials[2 * n_partials] (one per block),
 * for buffers that did not come out of uavhip_gae. */
int uavhip_adv_partials(const float* adv, int64_t n, double* partials, int32_t n_partials, uavhip_stream_t stream);

/* adv <- (adv - mean) / (std_unbiased + 1e-7) over n elements (ppo.py:94), mean/std folded in
 * fp64 from partials[2 * n_partials] (uavhip_gae or uavhip_adv_partials) in a fixed order, then
 * rounded to fp32 as the reference's fp32 tensors are. n_total = element count the partials
 * describe (0 -> n); with data-parallel ranks pass all-reduced partials and the global count so
 * every rank normalises with the statistics of the whole gathered batch. stats_out[2] =
 * {mean, std} (nullable, device f64). */
int uavhip_adv_normalize(float* adv, int64_t n, const double* partials, int32_t n_partials, int64_t n_total,
                         double* stats_out, uavhip_stream_t stream);

/* Policy-input windows [blocks][T][E][5][14] of a trajectory from its compact all-gather form
 * (uavhip/dist.py pack_compact; the data-parallel exchange of SURVEY.md 8e): per block, first
 * windows first[e][70] (the window at step 0), rows[t][e][14] (the row pushed at step t = window
 * slot 4; row 0 is read from the first window) and done flags done[(t * E + e) * done_stride] (f32,
 * nonzero = the episode ended at step t, so step t + 1 starts from a zero window,
 * uav_env.py:42-63,241-242). Blocks are block_stride floats apart in all three arrays (one rank's
 * payload each). Replaces shipping 70 window floats per transition in the gather: the deque only
 * shifts, so a window is the last 5 rows of its episode. */
int uavhip_windows_from_rows(const float* first, const float* rows, const float* done, int32_t done_stride,
                             int64_t block_stride, int32_t blocks, int32_t T, int32_t E, float* out,
                             uavhip_stream_t stream);

/* ---------------------------------------------------------------- policy forward (K4) */

/* Packed fp32 weights of TransformerActorCritic (transformer_net.py:67-144), produced by
 * uavhip/policy.py pack_weights() from the 50-key state_dict: each parameter at its
 * uavhip_policy_layout() offset, flat or in MFMA fragment order (uavhip_policy_tiling()). */
typedef struct uavhip_policy {
    const float* weights; /* packed buffer, layout = uavhip_policy_layout() offsets + split copies */
                          /* (n_floats = uavhip_policy_split_layout()) */
    int32_t n_floats;
    int32_t d_model, n_heads, d_ff, d_head_hidden; /* 128, 8, 256, 64 */
    int32_t actor_layers, critic_layers;           /* 1, 2 */
} uavhip_policy;

/* Offsets (in floats) of every parameter in the packed buffer, in state_dict key order
 * (see policy.py). Returns the total number of floats; offsets may be NULL. */
int32_t uavhip_policy_layout(int32_t* offsets, int32_t max_offsets);

/* The inference forward's packed buffer (uavhip_policy.weights / n_floats) holds, after the
 * uavhip_policy_layout() parameters, split copies of the GEMM weights that run on the f16 matrix
 * cores as fp32-accurate split products: weight `params[i]` (state_dict index, [R][K]) at float
 * offset `offsets[i]`, as two fp16 planes w1 = f16(w), w2 = f16((w - w1) * 2^11) in split fragment
 * order (blocks of 16 rows x 32 k: 1 KiB of w1 then 1 KiB of w2, lane = r%16 + 16 ((k%32)/8)
 * holding k%8 = 0..7). Returns the packed buffer's total floats; params / offsets may be NULL. */
int32_t uavhip_policy_split_layout(int32_t* params, int32_t* offsets, int32_t max_entries);

/* flat (state_dict order, uavhip_policy_layout offsets, every parameter row-major) -> packed
 * (the same with the uavhip_policy_tiling weights in MFMA fragment order, the split copies and the
 * range table), on the device. */
int uavhip_policy_pack(const float* flat, float* packed, uavhip_stream_t stream);

/* The range table that ends the packed buffer (its last n floats, n = the return value): the
 * split products multiply every activation operand by a power of two 2^-s before splitting it into
 * fp16 planes and the GEMM output by 2^s, with s from a rigorous bound on the operand's magnitude
 * (0 on realistic weights), so no ACTIVATION operand the reference's fp32 can hold leaves fp16's
 * range (a bound that overflows fp32 takes the largest exponent, s = 113). The weights themselves
 * are not scaled: their split copies hold f16(w), so a parameter of magnitude >= 65520 makes the
 * outputs non-finite (never silently wrong); max_abs is the caller's check for that.
 * The packed buffer's table holds the maxima (max |param| of each state_dict tensor, floats 0..49;
 * the rest zero; uavhip_policy_pack writes them, an UPDATE step refreshes them) and every kernel
 * derives the scales from them. NaN elements do not count in a maximum (the device reduces with
 * fmaxf; the ctypes mirror drops them the same way), so host and device tables agree for any
 * parameters. Host side: max_abs[50] (key order) -> table[n]: the maxima, the
 * per-token constants of layer 0 and the static operands' (2^-s, 2^s) pairs -- bitwise what the
 * kernels derive. Either pointer NULL: only returns n. */
int32_t uavhip_policy_range_table(const float* max_abs, float* table);

/* Per parameter (state_dict key order): the in-features K of the weight matrices stored in MFMA
 * fragment order, 0 for parameters stored flat. An [R][K] matrix W in fragment order puts
 * W[r][k] at ((r/16 * K/16 + k/16) * 64 + r%16 + 16 * ((k%16)/4)) * 4 + k%4, so each 16 x 16
 * block the kernel streams is 1 KiB contiguous. Returns the number of parameters (50). */
int32_t uavhip_policy_tiling(int32_t* kcols, int32_t max_params);

/* get_action / evaluate (transformer_net.py:96-144) for B windows states[B][5][14]:
 * actions_in NULL -> sample a ~ Categorical(softmax(logits)) with Philox(seed, c), counter
 * c = offset + (offset_dev ? *offset_dev : 0) + b (offset_dev: device u64, lets a captured
 * hipGraph draw fresh numbers on every replay); else evaluate the given actions. Outputs
 * (nullable): action_out [B] int8, logp [B], value [B], entropy [B], logits [B][2] (all f32).
 *
 * Sampling counter. c is a 64-bit sum (it wraps modulo 2^64). The draw of window b is word 0, r, of
 * philox4x32_10(counter = {(uint32_t)c, (uint32_t)(c >> 32), 0x5eed, 0x9e37},
 *               key = {(uint32_t)seed, (uint32_t)(seed >> 32)});
 * u = (r >> 8) * 2^-24, a 24-bit uniform in [0, 1) that fp32 holds exactly; with p0 = expf(l0 - lse)
 * the fp32 probability of action 0, a = u < p0 ? 0 : 1. A draw belongs to its counter alone, not to
 * the workgroup or lane that makes it. The same rule holds for uavhip_policy_forward_rows,
 * uavhip_rollout_step (b = e), uavhip_rollout_steps / _rollout_actor_steps / uavhip_decode_steps
 * (c = offset + t * offset_stride + (offset_dev ? *offset_dev : 0) + e at step t). tests/device_rng.py
 * restates it; tests/test_gpu_device_rng.py compares every draw of every entry point. */
int uavhip_policy_forward(const uavhip_policy* policy, const float* states, int32_t B, const int8_t* actions_in,
                          uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int8_t* action_out,
                          float* logp, float* value, float* entropy, float* logits, uavhip_stream_t stream);

/* Rollout fast path of uavhip_policy_forward for a SEQUENCE of windows in which window g + 1 is
 * window g shifted by one row plus a new last row (the observation deque, uav_env.py:241-242;
 * after an episode end the earlier rows are zero padding). rowproj (caller-owned, size
 * uavhip_policy_rowproj_floats(B)) keeps, per window, the layer-0 in_proj of the embeddings of
 * its rows (a 5-slot ring indexed by step mod 5) and Win . pos of both trunks, so the forward of
 * step g projects only the new row (transformer_net.py:57-63 is linear up to the in_proj after
 * the embedding ReLU). step = g (>= 0, +1 per call along the sequence); fill != 0 rebuilds rows
 * 0-3 and the pos table from states and the current weights: required on the first call, after
 * the weights change, and whenever states is not the previous call's window advanced by one
 * row. Outputs as uavhip_policy_forward, equal to it within fp32 rounding (Win (e + pos) + b is
 * evaluated as (Win e + b) + Win pos). */
int64_t uavhip_policy_rowproj_floats(int32_t B);
int uavhip_policy_forward_rows(const uavhip_policy* policy, const float* states, int32_t B, float* rowproj,
                               int32_t step, int32_t fill, const int8_t* actions_in, uint64_t seed, uint64_t offset,
                               const uint64_t* offset_dev, int8_t* action_out, float* logp, float* value,
                               float* entropy, float* logits, uavhip_stream_t stream);

/* The value head alone on the window-row ring (the rollout's bootstrap V(s_T) after the last step,
 * ppo.py:70-94's next value): uavhip_policy_forward_rows' value output, bitwise, from the critic
 * trunk and head only (no actor trunk, no sampling: about 2/3 of the forward). The actor's ring row
 * of this step is not written, so the next call on the sequence must pass fill != 0. */
int uavhip_policy_value_rows(const uavhip_policy* policy, const float* states, int32_t B, float* rowproj,
                             int32_t step, int32_t fill, float* value, uavhip_stream_t stream);

/* One rollout step in ONE launch (main_train.py:109-117: select_action, then env.step): the
 * window-row forward of uavhip_policy_forward_rows with sampling, followed in the same
 * workgroups by the env step (uavhip_env_step, T = 1) of env e with the action sampled for
 * window b = e. B = env->E; the same outputs as the two calls in sequence, bitwise: action_out,
 * logp, value [E] of the forward, obs_out [E][5][14] (the next windows; f32, or binary16 under
 * UAVHIP_ENV_OBS_F16), reward [E], done [E], info [E][UAVHIP_INFO_COUNT] (nullable) of the step.
 * Needs N, M <= 64 (one env per wave). Saves the T = 1 env launch's fixed cost (dispatch, the
 * state-load round, the store drain: ~7 of its ~10 us at 4096 envs). */
int uavhip_rollout_step(const uavhip_policy* policy, const uavhip_env* env, const float* states, float* rowproj,
                        int32_t step, int32_t fill, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                        int8_t* action_out, float* logp, float* value, int32_t auto_reset, float* obs_out,
                        double* reward, uint8_t* done, double* info, uavhip_stream_t stream);

/* n consecutive rollout steps in ONE launch (main_train.py:109-117 repeated n times): step t runs
 * uavhip_rollout_step on windows obs[t] with ring step `step` + t and sampling counters
 * offset + t * offset_stride + b, writing actions / logp / value / reward / done [t][E], info
 * [t][E][UAVHIP_INFO_COUNT] (nullable) and the next windows obs[t + 1]. obs is the time-major
 * [n + 1][E][5][14] f32 trajectory buffer (obs[0] = the current windows). Bitwise equal to n
 * uavhip_rollout_step calls. Every workgroup loops over the steps of its own 16 envs, so no
 * grid-wide synchronisation is involved; saves the per-launch tail and start-up of n - 1
 * launches. N, M <= 64; f32 observations (no UAVHIP_ENV_OBS_F16). */
int uavhip_rollout_steps(const uavhip_policy* policy, const uavhip_env* env, float* obs, float* rowproj,
                         int32_t step, int32_t n, int32_t fill, uint64_t seed, uint64_t offset,
                         uint64_t offset_stride, const uint64_t* offset_dev, int8_t* actions, float* logp,
                         float* value, int32_t auto_reset, double* reward, uint8_t* done, double* info,
                         uavhip_stream_t stream);

/* uavhip_rollout_steps with the critic taken off the step chain, in two launches. Sampling and the
 * env step read the actor's logits only, and the value of a window is read after the steps (GAE):
 *  - uavhip_rollout_actor_steps: the n steps with the ACTOR trunk and head only. Arguments as
 *    uavhip_rollout_steps without `value`; obs[t + 1], actions, logp, reward, done, info, the env
 *    state and the actor's ring rows are bitwise uavhip_rollout_steps'. fill != 0 rebuilds the ring
 *    rows of both trunks; after that the critic's ring rows are neither read nor written.
 *  - uavhip_value_steps: the critic trunk and head alone over the recorded windows of one deque
 *    sequence, obs [n + 1][B][5][14] f32 (the trajectory buffer after the steps): values [n][B] =
 *    V(obs[t]), t < n, and last_values [B] = V(obs[n]) (nullable: obs[n] is then not read). `step`
 *    is the ring step of obs[0]; it advances the critic's ring rows as the n (+ 1) steps of
 *    uavhip_rollout_steps (+ uavhip_policy_value_rows) would. fill != 0 rebuilds the ring rows from
 *    obs[0] first (not needed right after uavhip_rollout_actor_steps with fill on the same rowproj).
 *    The windows are taken in groups of five consecutive steps: per window the critic runs up to
 *    its last layer's attention, and that layer's out-projection, LayerNorms, FFN and the value
 *    head run once per group on the five windows' last tokens together. stash: device scratch of
 *    uavhip_value_steps_stash_floats(B) floats (contents unspecified before and after).
 *    The values are bitwise those of uavhip_rollout_steps / uavhip_policy_value_rows. */
int64_t uavhip_value_steps_stash_floats(int32_t B);
int uavhip_rollout_actor_steps(const uavhip_policy* policy, const uavhip_env* env, float* obs, float* rowproj,
                               int32_t step, int32_t n, int32_t fill, uint64_t seed, uint64_t offset,
                               uint64_t offset_stride, const uint64_t* offset_dev, int8_t* actions, float* logp,
                               int32_t auto_reset, double* reward, uint8_t* done, double* info,
                               uavhip_stream_t stream);
int uavhip_value_steps(const uavhip_policy* policy, const float* obs, int32_t B, int32_t n, float* rowproj,
                       int32_t step, int32_t fill, float* values, float* last_values, float* stash,
                       uavhip_stream_t stream);

/* ---------------------------------------------------------------- inference (decode) */

/* Decode an allocation with a trained policy: up to n_max steps of every env in ONE launch, each
 * step the ACTOR trunk and head of the window-row forward, an action, and the env step with
 * UAVHIP_STEP_HOLD -- no critic, no logp / value, no trajectory, no auto-reset. The critic's ring
 * rows are neither read nor written (a later forward of both trunks on this rowproj needs fill).
 *  - action of env e: greedy (a = l1 > l0, a tie gives 0) iff greedy_stride > 0 and
 *    e % greedy_stride == 0; else sampled as uavhip_rollout_steps samples, Philox counter
 *    offset + t * offset_stride + (offset_dev ? *offset_dev : 0) + e at the call's step t = 0, 1, ..
 *    (greedy_stride 1: all greedy; 0: all sampled; K: replica 0 of each scene of K replicas);
 *  - a finished env (istate[UAV_IDX] >= N) is held, and a workgroup (16 envs) leaves the step
 *    loop once all of its envs are finished;
 *  - obs2 [2][E][5][14] f32: the windows ping-pong, step `step` + t reads slot (step + t) & 1 and
 *    writes the other; the caller puts the current windows into slot step & 1;
 *  - step: the ring step of the first decoded step (as uavhip_rollout_steps; also picks the
 *    window slot). A continuation call passes the steps decoded so far and fill = 1;
 *  - steps [E] int32 (required): steps taken by env e since its reset, ADDED to (the caller zeroes
 *    it at a reset); finished [E] u8 (required): written; actions [n_max][E] int8 (nullable): the
 *    action trace of this call, -1 in the rows at or past the env's end; ep_return [E] f64
 *    (nullable): sum of rewards including the goal reward, ADDED to in step order.
 * N, M <= 64; f32 observations. */
int uavhip_decode_steps(const uavhip_policy* policy, const uavhip_env* env, float* obs2, float* rowproj,
                        int32_t step, int32_t n_max, int32_t fill, int32_t greedy_stride, uint64_t seed,
                        uint64_t offset, uint64_t offset_stride, const uint64_t* offset_dev, int8_t* actions,
                        int32_t* steps, uint8_t* finished, double* ep_return, uavhip_stream_t stream);

/* Best of K: envs are K replicas of E / K scenes, scene-major (e = s * K + k). Per scene s, the
 * FINISHED replica with the largest dstate[J] (lowest k on a tie): best [S] int32 = k, or -1 when no
 * replica finished (then J = 0, covered = 0, assignment all -1); J [S] f64; covered [S] int32 =
 * istate[N_COVERED]; assignment [S][N] int32 = tgt_id (of the replica's ACTIVE scene buffer) of each
 * UAV's target, -1 for none. Every output is required. */
int uavhip_select_best(const uavhip_env* env, int32_t K, int32_t* best, double* J, int32_t* covered,
                       int32_t* assignment, uavhip_stream_t stream);

/* Best-response local search on J(X) itself (k_refine, refine.hip): polish an allocation, build a
 * non-learned baseline (start from the empty assignment), or only score an assignment from
 * elsewhere (max_sweeps = 0). Row s < S uses the scene of env e = s * env_stride (its ACTIVE buffer;
 * env_stride = K right after uavhip_select_best with K replicas). With list-order targets
 * t = 0..M-1, P[u][t] = p_dmg[u][t] * p_pen[u] (the env step's pf), v = tgt_value, c = uav_cost,
 * w = prm[UAVHIP_PRM_OMEGA] and an assignment a[u] in {-1, 0..M-1}:
 *   J(a) = sum_t v[t] (1 - prod_{u: a[u] = t} (1 - P[u][t])) - w sum_{u: a[u] >= 0} c[u]
 * (_calc_J_X, uav_env.py:244-269). One sweep visits u = 0..N-1 in order, every move visible to the
 * next UAV: Q[t] = the product of (1.0 - P[w][t]) over the w != u with a[w] = t, ascending w, from
 * 1.0; g[t] = (v[t] * Q[t]) * P[u][t] - (w * c[u]) in that order of operations, not contracted;
 * g[-1] = 0.0; the candidate is the lowest index attaining the maximum over -1, 0, .., M-1; u moves
 * to it iff its gain is strictly greater than g[a[u]]. g[t] is u's marginal contribution to J, so J
 * never decreases in exact arithmetic. The search stops after a sweep without a move or after
 * max_sweeps sweeps.
 *  - assignment_in [S][N] int32 (nullable: every UAV starts at -1): target IDS (tgt_id, as
 *    uavhip_select_best writes them) or -1; an id that matches no tgt_id of the scene counts as -1
 *    and is counted in stats; of a duplicated id the lowest list index is taken;
 *  - assignment_out [S][N] int32 (required; may alias assignment_in): target ids or -1;
 *  - J [S] f64, covered [S] int32 = targets with at least one UAV (both required);
 *  - stats [S][4] int32 (nullable): sweeps run, moves made, 1 if the last sweep made no move (or
 *    max_sweeps = 0) else 0, invalid input ids.
 * Needs env_stride >= 1, S >= 1, (S - 1) * env_stride < E, max_sweeps >= 0. The full N <= 64,
 * M <= 128 range. The env's state and scene are only read. */
int uavhip_refine_assignments(const uavhip_env* env, int32_t env_stride, int32_t S, int32_t max_sweeps,
                              const int32_t* assignment_in, int32_t* assignment_out, double* J,
                              int32_t* covered, int32_t* stats, uavhip_stream_t stream);

/* Exchange-move local search on J(X) (k_search, search.hip): uavhip_refine_assignments' best-response
 * sweeps, which stop at the first allocation no single move improves, plus a second neighbourhood,
 * the pairwise exchange: UAVs i and j swap their targets, one of which may be "none". Notation as
 * above (list-order targets, P, v, c, w, a[u] in {-1, 0..M-1}); nothing contracted.
 *   g(u, x, Q) = 0.0                                   if x == -1
 *              = (v[x] * Q) * P[u][x] - (w * c[u])     otherwise
 *   Qo(u)      = the product of (1.0 - P[k][a[u]]) over the UAVs k != u with a[k] == a[u],
 *                ascending k, from 1.0   (1.0 when a[u] == -1)
 *
 *   a <- assignment_in converted exactly as uavhip_refine_assignments converts it; x <- 0
 *   repeat:
 *     PHASE: best-response sweeps from a, exactly uavhip_refine_assignments' sweep, until a sweep
 *            makes no move or max_sweeps sweeps of this phase have run. sweeps, moves accumulate over
 *            phases; phase_converged = 1 iff the phase ended on a sweep without a move, or
 *            max_sweeps == 0.
 *     if max_exchanges == 0: scan_clean = 0; stop                      (no scan is run)
 *     SCAN:  for every pair i < j with a[i] != a[j]   (s = a[i], t = a[j]; at most one of them is -1):
 *                d(i, j) = (g(j, s, Qo(i)) + g(i, t, Qo(j))) - (g(i, s, Qo(i)) + g(j, t, Qo(j)))
 *            in that order of operations. j is not on s and i is not on t, so Qo(i) / Qo(j) are the
 *            products over the other UAVs on s / t. The candidate is the pair with the largest d; of
 *            equal d, the lowest i, then the lowest j.
 *     if no pair has d > 0.0: scan_clean = 1; stop
 *     if x == max_exchanges:  scan_clean = 0; stop
 *     swap a[i], a[j]; x <- x + 1
 * d(i, j) is the change of J under the swap in exact arithmetic. The loop runs at most
 * max_exchanges + 1 phases, so it terminates whatever rounding does. J, covered and the id
 * conversion of the result are uavhip_refine_assignments' own.
 *  - env, env_stride, S, max_sweeps, assignment_in (nullable), assignment_out (required; may alias
 *    assignment_in), J, covered (required): as uavhip_refine_assignments, with the same bounds;
 *  - max_exchanges >= 0; with max_exchanges == 0 every output is bitwise
 *    uavhip_refine_assignments', and stats[:, :4] is its stats;
 *  - stats [S][6] int32 (nullable): sweeps run, moves made, phase_converged, invalid input ids,
 *    exchanges made, scan_clean.
 * The full N <= 64, M <= 128 range. The env's state and scene are only read; no allocation, no
 * atomics, no grid-wide synchronisation. */
int uavhip_search_assignments(const uavhip_env* env, int32_t env_stride, int32_t S, int32_t max_exchanges,
                              int32_t max_sweeps, const int32_t* assignment_in, int32_t* assignment_out,
                              double* J, int32_t* covered, int32_t* stats, uavhip_stream_t stream);

/* The exchange-move search under constraints (k_search_constrained, search_constrained.hip): pairs
 * that may not be flown, UAVs that keep the target they came with (a plan partly executed), and a
 * limit on the UAVs of one target. Notation, g, Qo, the id conversion, J, covered and the termination
 * argument are uavhip_search_assignments'; nothing contracted. The constraint arrays are indexed by
 * ROW s (not by env) and their columns are in LIST order, as p_dmg's; a NULL array constrains nothing:
 *   allowed  [S][N][M] u8   nonzero = UAV u may take list-order target t        (NULL: every pair)
 *   fixed    [S][N]    u8   nonzero = UAV u keeps its input target, or none      (NULL: no UAV)
 *   capacity [S][M]    i32  the most UAVs on list-order target t; < 0 counts as 0 (NULL: no limit)
 * With n[t] the UAVs counted on t so far:
 *
 *   START: a <- assignment_in converted exactly as uavhip_refine_assignments converts it (a fixed UAV
 *          whose id matches no tgt_id is fixed to none); n <- 0; dropped <- 0; fixed_conflicts <- 0
 *     pass 1, the fixed u in ascending order with a[u] >= 0: u keeps a[u] whatever the other
 *            constraints say;  fixed_conflicts += 1 if !allowed[u][a[u]];
 *            fixed_conflicts += 1 if n[a[u]] >= capacity[a[u]];  n[a[u]] += 1
 *     pass 2, the free u in ascending order with a[u] >= 0: if !allowed[u][a[u]] or
 *            n[a[u]] >= capacity[a[u]]: a[u] <- -1, dropped += 1; else n[a[u]] += 1
 *   PHASE: uavhip_refine_assignments' sweep with two changes. A fixed u is skipped: no visit, no
 *          move. For a free u the candidates are -1 and the targets t with allowed[u][t] and
 *          (t == a[u] or the number of OTHER UAVs on t < capacity[t]); among them the rule is the
 *          sweep's own: g[t] = (v[t] * Q[t]) * P[u][t] - (w * c[u]), the candidate is the lowest
 *          index attaining the maximum if that maximum is > 0.0, else -1 (gain 0.0), and u moves
 *          iff the gain is strictly greater than g[a[u]]. (a[u] of a free u is always a candidate.)
 *   SCAN:  uavhip_search_assignments' scan over the pairs i < j with both UAVs free, a[i] != a[j],
 *          (s == -1 or allowed[j][s]) and (t == -1 or allowed[i][t]), s = a[i], t = a[j]; d(i, j),
 *          its order of operations and the tie-break are unchanged. A swap keeps every target's
 *          count, so capacity is not looked at.
 *   The loop of phases, scans and exchanges, max_exchanges and max_sweeps are
 *   uavhip_search_assignments'.
 * Guarantees: every free UAV's output pair is allowed; no target holds more UAVs, free and fixed,
 * than max(capacity[t], its fixed UAVs); a fixed UAV leaves as it came. With the three arrays NULL,
 * and with neutral arrays (allowed all nonzero, fixed all zero, capacity >= N), every output is
 * bitwise uavhip_search_assignments', and stats[:, :6] is its stats.
 *  - env, env_stride, S, max_exchanges, max_sweeps, assignment_in (nullable), assignment_out (required;
 *    may alias assignment_in), J, covered (required): as uavhip_search_assignments, the same bounds;
 *  - stats [S][8] int32 (nullable): the six of uavhip_search_assignments, dropped, fixed_conflicts.
 * The full N <= 64, M <= 128 range. The env's state and scene and the constraint arrays are only
 * read; no allocation, no atomics, no grid-wide synchronisation. */
int uavhip_search_assignments_constrained(const uavhip_env* env, int32_t env_stride, int32_t S,
                                          int32_t max_exchanges, int32_t max_sweeps, const uint8_t* allowed,
                                          const uint8_t* fixed, const int32_t* capacity,
                                          const int32_t* assignment_in, int32_t* assignment_out, double* J,
                                          int32_t* covered, int32_t* stats, uavhip_stream_t stream);

/* The optimum of J(X) (k_exact_*, exact.hip): not a search but a subset DP over the UAVs, exact for
 * N <= UAVHIP_EXACT_MAX_N. J is a sum over targets of a function of the SET of UAVs on that target, so
 * with list-order targets t = 0..M-1, sets S, T of UAVs as N-bit integers (bit u = UAV u) and the
 * notation of uavhip_refine_assignments (P, v, c, w):
 *   val_t(T)   = v[t] (1 - prod_{u in T} (1 - P[u][t])) - w sum_{u in T} c[u]
 *   D_0[S]     = 0                                                        for every S
 *   D_{t+1}[S] = max over the feasible T <= S of  D_t[S \ T] + val_t(T)
 *   J*         = D_M[all UAVs]
 * 3^N steps per target. The feasible set is uavhip_search_assignments_constrained's guarantee: with F_t
 * the fixed UAVs on t (fixed[u] != 0 and assignment_in[u] converts to t) and "free" = not fixed, the set
 * T of UAVs on target t satisfies
 *   T >= F_t;   every free u in T has allowed[u][t];   |T| <= max(capacity[t], |F_t|)  (capacity < 0 as 0)
 * and a UAV fixed to none (its input -1, or an id that matches no tgt_id) is on no target. The three
 * arrays are that function's (indexed by row, columns in list order, each nullable); with all three
 * NULL this is the unconstrained problem. The feasible set is never empty (every fixed UAV on its
 * target and every free one on none is in it).
 * Arithmetic inside the DP is fp64, rounded in the kernel's own fixed order (not the order of J below).
 * Tie-break: where several feasible T attain the maximum of D_{t+1}[S] in that arithmetic, the smallest
 * T as an integer is taken; the result is then read back from t = M-1 down to 0 starting at S = all
 * UAVs (the UAVs of T = choice_t[S] go on t, S <- S \ T). Nothing depends on timing: no atomics, every
 * value is written by one lane in a fixed order, so two launches on the same inputs give bitwise equal
 * outputs.
 *  - env, env_stride, S, assignment_out, J, covered (all required): as uavhip_refine_assignments, the
 *    same row bounds; J, covered and the ids of the result come from the code uavhip_refine_assignments
 *    ends with, so J is bitwise uavhip_refine_assignments(assignment_out, max_sweeps = 0)'s and
 *    comparable with every other J of this library;
 *  - assignment_in [S][N] int32 (nullable): read only to learn where the fixed UAVs stand, converted
 *    as uavhip_refine_assignments converts it; required when fixed != NULL;
 *  - stats [S][2] int32 (nullable): invalid input ids, fixed_conflicts (as pass 1 of
 *    uavhip_search_assignments_constrained counts them);
 *  - workspace: device memory, 16-byte aligned, of workspace_bytes bytes, contents unspecified before
 *    and after. One row needs uavhip_exact_workspace_bytes(N, M, 1) bytes: two tables of 2^N doubles
 *    (D_t and D_{t+1}), the choice table [M][2^N] of uint16 and M 8-byte target masks (5 MiB + 256 B
 *    at 16 x 32). A workspace that holds fewer than S rows is no error: the rows run in chunks that
 *    fit, one after the other on `stream`. uavhip_exact_workspace_bytes returns -1 unless 1 <= N <= 16,
 *    1 <= M <= 128 and rows >= 1.
 * UAVHIP_EINVAL: N > UAVHIP_EXACT_MAX_N, the row bounds, a required output NULL, fixed without
 * assignment_in, a workspace that is NULL, misaligned or smaller than one row's need. Per chunk: one
 * launch that prepares the masks, M stage launches (the kernel boundary is the dependence between
 * stages) and one that reads the result back. Asynchronous on `stream`, capturable; no allocation, no
 * device or grid-wide synchronisation; the env and the inputs are only read. */
#define UAVHIP_EXACT_MAX_N 16
int64_t uavhip_exact_workspace_bytes(int32_t N, int32_t M, int32_t rows);
int uavhip_solve_exact(const uavhip_env* env, int32_t env_stride, int32_t S, const uint8_t* allowed,
                       const uint8_t* fixed, const int32_t* capacity, const int32_t* assignment_in,
                       int32_t* assignment_out, double* J, int32_t* covered, int32_t* stats, void* workspace,
                       int64_t workspace_bytes, uavhip_stream_t stream);

/* The optimum of J(X) over a NEIGHBOURHOOD (k_exact_free_*, exact_free.hip): the subset DP of
 * uavhip_solve_exact over a row's free UAVs only, everyone else held where assignment_in puts them, for
 * the full N <= 64, M <= 128. The DP's cost depends on the UAVs that may move (3^bits steps a target), and
 * a held UAV changes only the value of its target, so "these K <= 16 UAVs may go anywhere, the others
 * stay" is solved exactly at any N: a neighbourhood of (M + 1)^K assignments that contains every single
 * move, exchange, 3-cycle and ejection chain among the K. The rule is uavhip_solve_exact's word for word
 * -- the same feasible set, the same allowed [S][N][M] / fixed [S][N] / capacity [S][M] arrays (each
 * nullable), the same id conversion -- with these differences:
 *   FREE LIST of a row: the UAVs u with fixed[s][u] == 0 (all of them when fixed == NULL), ascending. The
 *     first K = min(max_free, N) of them are in the DP, and bit b of a set is the b-th of them. Any
 *     further free UAV is HELD exactly as a fixed one is: it keeps the target its input converts to,
 *     whatever the constraints say (fixed is device data: the host cannot refuse on it; stats column 3
 *     counts them).
 *   HELD UAVs (fixed, or free beyond the first K): with H_t the held UAVs on target t,
 *       q_fix[t] = prod_{u in H_t} (1.0 - P[u][t])      in ascending u, starting from 1.0
 *     and a stage is uavhip_solve_exact's with v[t] * q_fix[t] where that one uses v[t]:
 *       val_t(H_t + T) - val_t(H_t) = (v[t] q_fix[t]) (1 - prod_{u in T} (1 - P[u][t])) - w sum_{u in T} c[u]
 *     The free UAVs on t obey allowed and number at most max(capacity[t], |H_t|) - |H_t| (capacity < 0
 *     as 0; no limit without a capacity array).
 *   TIE-BREAK: of equal maxima the smallest T as an integer over the free-list bits; the result is read
 *     back from t = M-1 down, as there.
 *   A row with fewer than K free UAVs runs the same tables with dead high bits that no target may hold;
 *     the live bits are the lowest, the arithmetic of a set does not involve the dead ones, and no output
 *     depends on K beyond which UAVs are in the DP.
 * With N <= 16, fixed == NULL and max_free >= N every v[t] * 1.0 is v[t] and assignment_out, J, covered and
 * stats columns 0-1 are bitwise uavhip_solve_exact's. The result is never below the input's J beyond the
 * rounding of the DP's own sums when the input is feasible (the input is one of the assignments searched).
 *  - max_free: 1 <= max_free <= UAVHIP_EXACT_FREE_MAX;
 *  - env, env_stride, S, assignment_out, J, covered (all required): as uavhip_solve_exact; J, covered and
 *    the ids come from the code uavhip_refine_assignments ends with, so J is bitwise
 *    uavhip_refine_assignments(assignment_out, max_sweeps = 0)'s;
 *  - assignment_in [S][N] int32 (nullable: the empty start, every held UAV on none): where the held
 *    UAVs stand; a free UAV's input is not looked at. Required when fixed != NULL;
 *  - stats [S][4] int32 (nullable): invalid input ids; fixed_conflicts, counted over the held UAVs as
 *    pass 1 of uavhip_search_assignments_constrained counts them over the fixed ones; free UAVs in the
 *    DP; free UAVs held by overflow;
 *  - workspace: device memory, 16-byte aligned, contents unspecified before and after. One row needs
 *    uavhip_exact_free_workspace_bytes(K, M, 1) bytes -- uavhip_solve_exact's layout with K in place of N:
 *    two tables of 2^K doubles, the choice table [M][2^K] of uint16, then M 16-byte target records (the
 *    sets, the capacity left, v q_fix) and the 16-byte free list (1088 KiB + 2064 B at K = 12, M = 128).
 *    A workspace that holds fewer than S rows is no error: the rows run in chunks. That function returns
 *    -1 unless 1 <= max_free <= 16, 1 <= M <= 128 and rows >= 1.
 * Nothing depends on timing: no atomics, one lane writes each value, two calls give bitwise equal outputs.
 * UAVHIP_EINVAL: the row bounds, max_free out of range, a required output NULL, fixed without
 * assignment_in, a workspace that is NULL, misaligned or smaller than one row's need. Per chunk one
 * prepare launch, M stage launches, one read-back launch. Asynchronous on `stream`, capturable; no
 * allocation, no device or grid-wide synchronisation; the env and the inputs are only read. */
#define UAVHIP_EXACT_FREE_MAX 16
int64_t uavhip_exact_free_workspace_bytes(int32_t max_free, int32_t M, int32_t rows);
int uavhip_solve_exact_free(const uavhip_env* env, int32_t env_stride, int32_t S, int32_t max_free,
                            const uint8_t* allowed, const uint8_t* fixed, const int32_t* capacity,
                            const int32_t* assignment_in, int32_t* assignment_out, double* J, int32_t* covered,
                            int32_t* stats, void* workspace, int64_t workspace_bytes, uavhip_stream_t stream);

/* The free set of one round of a large-neighbourhood search (k_neighbourhood_pick, exact_free.hip),
 * chosen on device so that a loop of pick + uavhip_solve_exact_free needs no host synchronisation.
 * Writes fixed_out [S][N] uint8: 1 = held, 0 = free -- uavhip_solve_exact_free's `fixed`.
 *   KEYS of row s:  ku[u] = word (u & 3) of philox4x32_10(counter = {u >> 2, round, s, 0x4E424855},
 *                           key = {(uint32_t)seed, (uint32_t)(seed >> 32)}),
 *                   kt[t] = the same with 0x4E424854 over the target's LIST index t
 *     (the Philox of uavhip_search_multistart).
 *   The UAVs with fixed_in[s][u] != 0 are always held and never counted in K. The others are sorted by
 *   the mode's key, ascending, and the first min(K, their number) become free:
 *     UAVHIP_NBH_RANDOM:   (ku[u], u);
 *     UAVHIP_NBH_TARGETS:  (g[u], ku[u], u), with g[u] = 0 for a UAV whose assignment converts to none
 *       (-1, or an id of no target) and otherwise 1 + the rank of kt[a[u]] among the M target keys, ties
 *       by lower index: the idle UAVs first, then the whole crews of randomly chosen targets.
 *  - assignment [S][N] int32 (nullable: every UAV idle): target ids or -1, read in TARGETS mode only and
 *    converted as uavhip_refine_assignments converts them; fixed_in [S][N] uint8 (nullable);
 *    fixed_out (required) may alias fixed_in.
 * Deterministic; the env and the inputs are only read. UAVHIP_EINVAL: the row bounds, K outside
 * 1..UAVHIP_EXACT_FREE_MAX, a mode that is neither, fixed_out NULL. One launch, one wave per row,
 * asynchronous on `stream`, capturable. */
#define UAVHIP_NBH_RANDOM 0
#define UAVHIP_NBH_TARGETS 1
int uavhip_neighbourhood_pick(const uavhip_env* env, int32_t env_stride, int32_t S, int32_t K, int32_t mode,
                              uint32_t round, uint64_t seed, const int32_t* assignment, const uint8_t* fixed_in,
                              uint8_t* fixed_out, uavhip_stream_t stream);

/* Multi-start search (k_search_multistart / k_multistart_select, search_multistart.hip): per row the
 * best of R independent runs ("replicas") of uavhip_search_assignments_constrained's rule, replica 0
 * from assignment_in and the others from random full assignments. A local search stops at the first
 * local optimum it meets; restarts are the simplest way past it and parallelise over replicas. Rows,
 * env_stride, allowed [S][N][M], fixed [S][N], capacity [S][M] and assignment_in [S][N] are exactly
 * uavhip_search_assignments_constrained's, each nullable (NULL constrains nothing; a NULL start is
 * the empty assignment).
 *   REPLICA r of row s, 0 <= r < R: that function's whole rule -- conversion, the two start passes,
 *     the phases, the scans and the exchanges, with the caps max_exchanges and max_sweeps PER REPLICA
 *     -- from start_r:
 *       start_0 = assignment_in[s], so replica 0 is that function's result bit for bit;
 *       r >= 1: assignment_in[s] is converted as ever (stats column 3, the invalid ids, is therefore
 *         the same in every replica). A UAV u with fixed[s][u] != 0 keeps what the conversion gave
 *         it. Every other UAV starts on the target of LIST index
 *             t = (x * M) >> 32                                   (a 64-bit product, 0 <= t < M)
 *         with x = word (u & 3) of
 *             philox4x32_10(counter = {u >> 2, r, s, 0x5354524D}, key = {(uint32_t)seed, (uint32_t)(seed >> 32)})
 *         -- the Philox4x32-10 of Salmon et al. (multipliers D2511F53 / CD9E8D57, key increments
 *         9E3779B9 / BB67AE85, ten rounds; words in the order of the reference implementation's
 *         output). A random start is a list index and needs no id conversion; what the constraints
 *         do not admit is dropped by the rule's own pass 2.
 *   CHOICE: with J_r the double the rule's scoring forms for replica r (the J of
 *     uavhip_refine_assignments), r* = the lowest r among the replicas whose J_r is the largest;
 *     "largest" and "equal" compare the doubles themselves.
 *  - R: 1 <= R <= UAVHIP_MULTISTART_MAX_R, and S * R <= 2^30; seed: the Philox key;
 *  - env, env_stride, S, max_exchanges, max_sweeps, assignment_in (nullable), assignment_out (required;
 *    may alias assignment_in), J, covered (required): as uavhip_search_assignments_constrained, the same
 *    bounds; they hold replica r*'s results, so J[s] >= that function's J[s] in every row;
 *  - stats [S][10] int32 (nullable): columns 0-7 replica r*'s eight counters of the constrained search,
 *    column 8 r*, column 9 the number of replicas whose J is strictly greater than replica 0's;
 *  - J_all [S][R] f64 (nullable): J_r of every replica;
 *  - workspace: device memory, 16-byte aligned, of at least uavhip_multistart_workspace_bytes(S, R, N)
 *    bytes (44 + 4 N bytes per replica: J, covered, N ids, eight counters), contents unspecified before
 *    and after. That function returns -1 unless 1 <= S, 1 <= R <= 1024, 1 <= N <= 64, S * R <= 2^30.
 * Guarantees: those of uavhip_search_assignments_constrained, for every replica. Two calls with the same
 * arguments give bitwise equal outputs: one wave per replica, every value written by one lane.
 * UAVHIP_EINVAL: the row bounds, a cap < 0, R out of range, a required output NULL, a workspace that is
 * NULL, misaligned or too small. Two launches -- S * R waves of the search, one per (row, replica), then
 * one wave per row that chooses -- asynchronous on `stream`, capturable; the full N <= 64, M <= 128
 * range; no allocation, no atomics, no device or grid-wide synchronisation; the env's state and scene
 * and the inputs are only read. */
#define UAVHIP_MULTISTART_MAX_R 1024
int64_t uavhip_multistart_workspace_bytes(int32_t S, int32_t R, int32_t N);
int uavhip_search_multistart(const uavhip_env* env, int32_t env_stride, int32_t S, int32_t R, uint64_t seed,
                             int32_t max_exchanges, int32_t max_sweeps, const uint8_t* allowed,
                             const uint8_t* fixed, const int32_t* capacity, const int32_t* assignment_in,
                             int32_t* assignment_out, double* J, int32_t* covered, int32_t* stats, double* J_all,
                             void* workspace, int64_t workspace_bytes, uavhip_stream_t stream);

/* Multi-start search from GIVEN starts (the same two kernels): uavhip_search_multistart with the first R0
 * of a row's R replicas started from R0 assignments of the caller's -- the K decoded replicas of a
 * policy, say -- and the other R - R0 from random full assignments as ever. Everything not named here is
 * uavhip_search_multistart's: rows, env_stride, allowed [S][N][M], fixed [S][N], capacity [S][M] (each
 * nullable), the caps per replica, CHOICE, stats [S][10], J_all [S][R], the workspace and
 * uavhip_multistart_workspace_bytes(S, R, N).
 *   starts [S][R0][N] int32: target ids or -1, R0 starts per row, start k of row s at starts[(s * R0 + k) * N].
 *   FIXED0: for a row s, fixed0[u] = the list index starts[s][0][u] converts to (-1 for -1 and for an id
 *     that matches no tgt_id), for the UAVs u with fixed[s][u] != 0. EVERY replica of the row holds those
 *     UAVs there, so all replicas of a row solve the same constrained problem and their J are comparable;
 *     what starts[s][r][u], r >= 1, says of a fixed u is not read.
 *   GIVEN REPLICA r, 0 <= r < R0:
 *       start_r[u] = fixed0[u] for a fixed u, else starts[s][r][u] converted;
 *     the conversion is uavhip_refine_assignments' own (of a duplicated id the lowest list index; an id
 *     that matches no tgt_id counts as -1 and is counted). From start_r the replica is
 *     uavhip_search_assignments_constrained's whole rule -- the two start passes, the phases, the scans
 *     and the exchanges -- bit for bit that function's result for assignment_in = start r with row 0's
 *     ids written over the fixed UAVs. stats column 3 of a given replica counts the invalid ids of the
 *     start it was actually given: starts[s][r][u] over its free u, starts[s][0][u] over the fixed u.
 *   RANDOM REPLICA r, R0 <= r < R: exactly replica r of uavhip_search_multistart for the same s and seed
 *     with assignment_in[s] = starts[s][0]: all of starts[s][0] is converted (and counted in column 3), a
 *     fixed UAV keeps fixed0[u], every other UAV starts on list index t = (x * M) >> 32, x = word (u & 3)
 *     of philox4x32_10(counter = {u >> 2, r, s, 0x5354524D}, key = {(uint32_t)seed, (uint32_t)(seed >> 32)}).
 *     The counter holds r itself: a random replica's J depends on r, s and seed, not on how many given
 *     starts precede it.
 *  - R0: 1 <= R0 <= R <= UAVHIP_MULTISTART_MAX_R. starts == NULL is allowed only with R0 == 1 (the empty
 *    start). With R0 == 1 every output is bitwise uavhip_search_multistart's with assignment_in = starts;
 *  - assignment_out (required): may alias starts only when R0 == 1 (then [S][N] on both sides, and the
 *    kernel boundary is the dependence); with R0 > 1 the two must not overlap;
 *  - column 9 of stats counts the replicas strictly above replica 0's J, given and random alike; r* < R0
 *    says that a given start won.
 * Guarantees: those of uavhip_search_assignments_constrained for every replica, with the fixed UAVs where
 * starts[s][0] puts them; J[s] >= the J of every given start's own constrained search; two calls with the
 * same arguments give bitwise equal outputs.
 * UAVHIP_EINVAL: R0 < 1, R0 > R, starts == NULL with R0 > 1, and everything uavhip_search_multistart
 * refuses. Two launches, asynchronous on `stream`, capturable; the full N <= 64, M <= 128 range; no
 * allocation, no atomics, no device or grid-wide synchronisation; the env's state and scene and the
 * inputs are only read. */
int uavhip_search_multistart_from(const uavhip_env* env, int32_t env_stride, int32_t S, int32_t R, int32_t R0,
                                  uint64_t seed, int32_t max_exchanges, int32_t max_sweeps, const uint8_t* allowed,
                                  const uint8_t* fixed, const int32_t* capacity, const int32_t* starts,
                                  int32_t* assignment_out, double* J, int32_t* covered, int32_t* stats,
                                  double* J_all, void* workspace, int64_t workspace_bytes, uavhip_stream_t stream);

/* Teacher-forced episodes (k_teacher_steps, teacher.hip): walk every env along a GIVEN allocation,
 * up to n_max steps in ONE launch, and record the window each action was decided on, the action and
 * the env's own reward / done / info -- the training data of uavhip.imitate. The action of a step is
 * a function of the env's pointer (u, t) alone:
 *   a = (teach[u] == t) ? 1 : 0,   teach[u] = the list index of UAV u's target, or -1,
 * and the step is the env step with UAVHIP_STEP_HOLD (bitwise the step uavhip_env_step takes for the
 * same action). The env decides: an assign it rejects (r(X') < r(X)) walks on to t + 1, and that UAV
 * stays unassigned for the rest of the episode (its teacher index is behind the pointer).
 *  - assignment [E][N] int32 (required): target IDS (tgt_id of the env's ACTIVE scene buffer, as
 *    uavhip_select_best / uavhip_refine_assignments write them) or -1, converted as
 *    uavhip_refine_assignments converts them: an id that matches no tgt_id counts as -1 and is
 *    counted in stats; of a duplicated id the lowest list index is taken;
 *  - every env starts from its CURRENT state (the caller has reset it); an env already finished
 *    (istate[UAV_IDX] >= N) is held from step 0; afterwards the env is stepped -- it holds the
 *    allocation it accepted, as after a decode;
 *  - outputs, time-major, each nullable: obs [n_max][E][5][14] f32 -- obs[t] is the window step t's
 *    action was decided on: obs[0] the env's own window at entry, obs[t + 1] what step t emitted;
 *    actions [n_max][E] int8 (0 / 1); reward [n_max][E] f64; done [n_max][E] u8;
 *    info [n_max][E][UAVHIP_INFO_COUNT] f64. In the rows at or past an env's end (held rows): a zero
 *    window, action -1, reward 0, done 1, info 0;
 *  - steps [E] int32 (required): ADDED to; finished [E] u8 (required): written; ep_return [E] f64
 *    (nullable): the rewards ADDED to it in step order -- all three as uavhip_decode_steps;
 *  - stats [E][2] int32 (nullable), written: teacher assigns the env rejected in this call (action-1
 *    steps that left the allocation unchanged, reward 0), invalid input ids.
 * Needs n_max >= 1 (N * M bounds every episode). The full N <= 64, M <= 128 range; f32 observations
 * only (UAVHIP_EINVAL under UAVHIP_ENV_OBS_F16). */
int uavhip_teacher_steps(const uavhip_env* env, const int32_t* assignment, int32_t n_max, float* obs,
                         int8_t* actions, double* reward, uint8_t* done, double* info, int32_t* steps,
                         uint8_t* finished, double* ep_return, int32_t* stats, uavhip_stream_t stream);

/* On-policy expert labels (k_expert_steps, expert.hip): walk every env along an ARBITRARY action
 * trace, up to n_max steps in ONE launch, and record per step the window the action was decided on,
 * the action taken and what the state-wise expert would have done in that state -- the relabelling
 * step of DAgger (uavhip.imitate, source "dagger"). The expert at the env's pointer (u, t), with
 * list-order targets t' = 0..M-1, v = tgt_value, c = uav_cost, w = prm[UAVHIP_PRM_OMEGA]:
 *   P[x][t'] = p_dmg[x][t'] * p_pen[x]                                  (the env step's pf);
 *   Q[t']    = the product of (1.0 - P[x][t']) over the UAVs x currently locked on t', ascending x,
 *              from 1.0 (the env's nh_final[t'] is that product bit for bit: the walk locks UAVs in
 *              ascending order, at most once each);
 *   g[t']    = (v[t'] * Q[t']) * P[u][t'] - (w * c[u])   in that order of operations, not contracted;
 *   label    = 1 iff g[t] > 0.0 and g[t'] <= g[t] for every t < t' < M, else 0;
 *   margin   = g[t] - max(0.0, max_{t' > t} g[t'])       (the inner max over nothing counts as 0.0).
 * g[t'] is u's marginal contribution to J (uavhip_refine_assignments) on the targets the walk can
 * still reach; following the labels from a reset is one best-response sweep from the empty
 * assignment: the allocation of uavhip_refine_assignments(NULL, max_sweeps = 1).
 *  - the action taken: env e follows the expert (action = label) iff actions_in == NULL or
 *    (follow != NULL and follow[e] != 0); otherwise it takes actions_in[step][e] (actions_in
 *    [n_max][E] int8, follow [E] u8; follow without actions_in is refused). A value outside {0, 1}
 *    on a live env ends its trace: the env is held from that step on, finished[e] stays 0 and
 *    stats[e][2] = 1 (an env that has finished ignores its trace: uavhip_decode_steps' -1 rows);
 *  - the step is the env step with UAVHIP_STEP_HOLD, bitwise uavhip_env_step's for the same action;
 *    every env starts from its CURRENT state, an env already finished is held from step 0;
 *  - outputs, time-major, each nullable: obs [n_max][E][5][14] f32 (obs[t] = the window step t's
 *    action was decided on, uavhip_teacher_steps' convention); actions [n_max][E] int8 (the action
 *    taken); labels [n_max][E] int8; margin [n_max][E] f64; reward [n_max][E] f64; done [n_max][E]
 *    u8. Held rows (at or past the env's end, or past its trace's end): a zero window, action -1,
 *    label -1, margin 0, reward 0, done 1;
 *  - steps [E] int32 (required): ADDED to; finished [E] u8 (required): written; ep_return [E] f64
 *    (nullable): the rewards ADDED to it in step order -- as uavhip_teacher_steps;
 *  - stats [E][3] int32 (nullable), written: assigns the env rejected in this call, steps whose
 *    action differs from the label, 1 if the trace ended on a live env else 0.
 * Needs n_max >= 1. The full N <= 64, M <= 128 range; f32 observations only (UAVHIP_EINVAL under
 * UAVHIP_ENV_OBS_F16). */
int uavhip_expert_steps(const uavhip_env* env, const int8_t* actions_in, const uint8_t* follow, int32_t n_max,
                        float* obs, int8_t* actions, int8_t* labels, double* margin, double* reward, uint8_t* done,
                        int32_t* steps, uint8_t* finished, double* ep_return, int32_t* stats, uavhip_stream_t stream);

/* ---------------------------------------------------------------- PPO update (K5) */

/* One clipped-PPO minibatch step of agents/ppo.py:96-169 (evaluate -> surrogate / clipped value
 * / entropy loss -> backward -> clip_grad_norm_(1.0) -> Adam with the four parameter groups of
 * ppo.py:17-22), as hand-written kernels: fp32-accurate split-product GEMMs on the f16 MFMA for the
 * encoder layers (forward / input gradients two-plane, weight gradients three-plane) and f32 MFMA
 * GEMMs for the embeddings and heads
 * (forward, input gradients, split-K weight gradients), fused residual+LayerNorm, attention,
 * heads+loss, and a fused clip+Adam. Parameters, gradients and the Adam moments are FLAT
 * buffers in the plain (not fragment-order) uavhip_policy_layout() layout; the torch module's
 * parameters can be views of `params`. */
typedef struct uavhip_ppo {
    float* params;       /* [n_floats] */
    float* grads;        /* [n_floats] this rank's gradient contribution (written by BACKWARD) */
    float* adam_m;       /* [n_floats] exp_avg */
    float* adam_v;       /* [n_floats] exp_avg_sq */
    double* adam_step;   /* [1] device step counter (shared by all groups) */
    float* workspace;    /* [uavhip_ppo_workspace_floats(minibatch)], zero-filled before first use */
    float* loss_sums;    /* [4] written by FORWARD: sums over this rank's samples of min(s1, s2),
                            (v - R)^2, (v_clip - R)^2, entropy; BACKWARD reads them (all-reduced);
                            FORWARD | BACKWARD in one call: summed and written by the backward */
    double* stats;       /* [4] += loss_actor, loss_critic, entropy, 1 per step (nullable) */
    int32_t n_floats;
    int32_t minibatch;   /* samples per step on this rank, multiple of 64 */
    int32_t global_minibatch; /* samples per step over all ranks (0: = minibatch) */
    /* torch.optim.Adam's hyper-parameters as torch holds them (Python floats = doubles): the bias
       corrections and step size are formed in double and the per-element coefficients rounded to
       float once, as torch's single-tensor Adam does -- its path for CPU tensors, where the reference's
       fixtures were recorded (agents/ppo.py:17-22); torch's CUDA default (foreach) differs by one
       rounding per element (train.hip k_adam) */
    double lr_actor, lr_critic, beta1, beta2, adam_eps; /* 2e-4, 1e-3, 0.9, 0.999, 1e-8 */
    float eps_clip, max_grad_norm, value_coef, entropy_coef; /* 0.2, 1.0, 0.5, 0.01 */
    int32_t flags;       /* UAVHIP_PPO_* variant bits below (0 = the measured defaults); any other
                            bit is UAVHIP_EINVAL. The workspace size does not depend on them */
} uavhip_ppo;

/* uavhip_ppo_step phases (bit mask). A data-parallel step over R ranks runs FORWARD,
 * all-reduces loss_sums (sum), runs BACKWARD (gradients scaled by 1 / global_minibatch, so their
 * sum over ranks is the global minibatch's gradient), all-reduces grads (sum), runs UPDATE. */
enum uavhip_ppo_phase {
    UAVHIP_PPO_FORWARD = 1,
    UAVHIP_PPO_BACKWARD = 2,
    UAVHIP_PPO_UPDATE = 4,   /* clip_grad_norm_ on grads + Adam */
    UAVHIP_PPO_FULL = 7,
    UAVHIP_PPO_PACKED = 8    /* with FORWARD: the workspace's packed weight copies are current (an
                                UPDATE on this workspace refreshes them with the new parameters,
                                and nothing changed the parameters since): skip the repack */
};

/* uavhip_ppo.flags (bit mask): each bit forces the other of two kernel paths that compute the same
 * step, for comparisons and traces. 0 is the measured default everywhere. */
enum uavhip_ppo_flag {
    UAVHIP_PPO_NO_POS_SPLIT = 1,     /* the 16-samples-per-workgroup forward / backward (K6) even at the
                                        minibatches that run the position split (K7) by default (0)   */
    UAVHIP_PPO_NO_TRUNK_SPLIT = 2,   /* actor and critic trunk in the same workgroups even at the
                                        minibatches that run them side by side by default (0)         */
    UAVHIP_PPO_WGRAD_STREAM_K = 4,   /* the stream-K weight-gradient schedule at every size; default
                                        (0): chunked from 64 k-slabs (2048 rows) on                   */
    UAVHIP_PPO_FIXED_ORDER_FWD = 8,  /* every workgroup of the training forward runs the actor trunk
                                        first; default (0): the order mixed across workgroups         */
    UAVHIP_PPO_FIXED_ORDER_BWD = 16, /* every workgroup of the backward runs the critic trunk first;
                                        default (0): the order mixed across workgroups                */
    UAVHIP_PPO_NO_GRAD_PRESCALE = 32,/* the backward without its power-of-two gradient pre-scale;
                                        default (0): scaled by the power of two >= global_minibatch   */
    UAVHIP_PPO_FLAGS_ALL = 63
};

/* Floats of workspace one step needs at `minibatch` samples. */
int64_t uavhip_ppo_workspace_floats(int32_t minibatch);

/* Minibatch rows idx[minibatch] (int32, into the trajectory buffers) of states[n][5][14],
 * actions[n] (int8), old_logp / old_values / returns / advantages [n] (f32); idx[i] < 0 marks a
 * padding row that adds nothing to loss_sums or grads (a rank's share of a global minibatch drawn
 * over the ranks' own trajectory shards varies from step to step); `phases` a mask of
 * uavhip_ppo_phase (UAVHIP_PPO_FULL on one GPU; FORWARD | BACKWARD leaves the raw gradients in
 * ppo->grads). BACKWARD needs the workspace FORWARD filled for the same rows. */
int uavhip_ppo_step(const uavhip_ppo* ppo, const float* states, const int8_t* actions, const float* old_logp,
                    const float* old_values, const float* returns, const float* advantages, const int32_t* idx,
                    int32_t phases, uavhip_stream_t stream);

/* The four hyper-parameters a schedule changes during a run, as a device buffer hyper[UAVHIP_HP_COUNT]
 * of doubles: values in device memory can change between replays of a captured graph that holds the
 * step, by-value kernel arguments cannot. */
enum uavhip_ppo_hyper {
    UAVHIP_HP_LR_ACTOR = 0,   /* read as a double where Adam's step scalars are formed (once per UPDATE,
                                 by the block that advances adam_step), as ppo->lr_actor is            */
    UAVHIP_HP_LR_CRITIC,      /* likewise, for ppo->lr_critic                                          */
    UAVHIP_HP_ENTROPY_COEF,   /* used as (float)hyper[i] (one double -> float rounding) by BACKWARD     */
    UAVHIP_HP_EPS_CLIP,       /* used as (float)hyper[i] by FORWARD (the loss sums) and BACKWARD        */
    UAVHIP_HP_COUNT
};

/* uavhip_ppo_step with the four values of uavhip_ppo_hyper read from `hyper` (device memory) by the
 * kernels when they RUN, not when they are launched or captured. hyper == NULL: exactly
 * uavhip_ppo_step (which is this call with NULL). hyper != NULL: ppo->lr_actor, lr_critic,
 * entropy_coef and eps_clip are ignored, in every phase (pass the same buffer to the FORWARD,
 * BACKWARD and UPDATE calls of a phase-split step); value_coef, max_grad_norm, the betas and
 * adam_eps stay by value. A buffer holding the descriptor's own values (the floats widened to
 * double) gives bitwise the by-value step; no launch is added in either mode. The buffer must stay
 * valid and unchanged while a step, or a captured graph holding one, is in flight: write it
 * stream-ordered between steps / replays. The values are not validated on the device (the caller
 * does: finite, learning rates and entropy_coef >= 0, eps_clip > 0; uavhip/train.py set_hyper). */
int uavhip_ppo_step_hyper(const uavhip_ppo* ppo, const double* hyper, const float* states, const int8_t* actions,
                          const float* old_logp, const float* old_values, const float* returns,
                          const float* advantages, const int32_t* idx, int32_t phases, uavhip_stream_t stream);

/* Update diagnostics of a batch of n samples (csrc/ppo_diag.hip), out[UAVHIP_DIAG_COUNT] f64. With
 * d_i = (double)new_logp_i - (double)old_logp_i and r_i = exp(d_i), all arithmetic in double: */
enum uavhip_diag {
    UAVHIP_DIAG_APPROX_KL = 0,   /* mean of (r_i - 1) - d_i                                         */
    UAVHIP_DIAG_CLIP_FRAC,       /* share of samples with |r_i - 1| > eps_clip (ppo.py:137's clamp)  */
    UAVHIP_DIAG_RATIO_MAX,       /* max of r_i (a NaN ratio is skipped: it shows in NONFINITE)       */
    UAVHIP_DIAG_RATIO_MEAN,      /* mean of r_i                                                      */
    UAVHIP_DIAG_VALUE_CLIP_FRAC, /* share with |new_value_i - old_value_i| > eps_clip (ppo.py:143)   */
    UAVHIP_DIAG_EXPLAINED_VAR,   /* 1 - Var(R - V_old) / Var(R); NaN when Var(R) == 0                */
    UAVHIP_DIAG_NONFINITE,       /* number of samples whose d_i is not finite                        */
    UAVHIP_DIAG_RETURN_VAR,      /* Var(R), population variance (exactly 0 for constant returns)     */
    UAVHIP_DIAG_RESIDUAL_VAR,    /* Var(R - V_old), population variance                              */
    UAVHIP_DIAG_COUNT
};

/* Doubles of the partials buffer uavhip_ppo_diagnostics needs for n samples (-1 for n < 1). */
int32_t uavhip_ppo_diagnostics_partials(int64_t n);

/* old_logp / new_logp / old_value / new_value / returns [n] f32. Two launches: per-block partials in
 * a fixed order (no atomics), then one block that merges them in index order, so the results are
 * bitwise repeatable and the call can be captured. The variances carry (count, mean, M2) per
 * partial, merged with the pairwise update formula. Non-finite inputs propagate into the sums and
 * are counted; nothing is clamped. partials: caller-owned, partials_doubles >=
 * uavhip_ppo_diagnostics_partials(n). */
int uavhip_ppo_diagnostics(const float* old_logp, const float* new_logp, const float* old_value,
                           const float* new_value, const float* returns, int64_t n, double eps_clip,
                           double* partials, int32_t partials_doubles, double* out, uavhip_stream_t stream);

/* ---------------------------------------------------------------- episode metrics */

/* Per-episode sums main_train.py logs (:122-136, :161-195), one record per finished episode. */
enum uavhip_ep {
    UAVHIP_EP_ENV = 0,       /* env index                                              */
    UAVHIP_EP_EPISODE,       /* info EPISODE of the finishing step                     */
    UAVHIP_EP_STEPS,         /* ep_steps                                               */
    UAVHIP_EP_REWARD,        /* current_ep_reward (sum of rewards)                     */
    UAVHIP_EP_Q0,            /* value of the episode's first state (current_q0)        */
    UAVHIP_EP_J_SUM,         /* ep_total_J (sum of info J_val)                         */
    UAVHIP_EP_MAX_COV,       /* ep_max_cov (max num_assigned)                          */
    UAVHIP_EP_ACTION1,       /* ep_action1_cnt                                         */
    UAVHIP_EP_VALID,         /* ep_valid_cnt (action 1 and is_valid_action)            */
    UAVHIP_EP_PDMG_SUM,      /* ep_total_p_dmg (steps with num_assigned > 0)           */
    UAVHIP_EP_PFINAL_SUM,    /* ep_total_p_final                                       */
    UAVHIP_EP_ASSIGN_STEPS,  /* ep_steps_with_assign                                   */
    UAVHIP_EP_COUNT
};

/* Walk a [T][E] rollout chunk (reward f64, done u8, action i8, info [T][E][UAVHIP_INFO_COUNT],
 * value f32 = V(obs[t])) per env in time order, continuing the episodes in acc[E][UAVHIP_EP_COUNT]
 * (zero-initialised once; carries unfinished episodes across chunks). Every finished episode is
 * appended to records[max_records][UAVHIP_EP_COUNT] at slot atomicAdd(n_records, 1) (slots past
 * max_records are counted but dropped). Sums run in step order in fp64, as the reference's. */
int uavhip_episode_stats(const double* reward, const uint8_t* done, const int8_t* action, const double* info,
                         const float* value, int32_t T, int32_t E, double* acc, double* records,
                         int32_t max_records, uint32_t* n_records, uavhip_stream_t stream);

/* ---------------------------------------------------------------- N > 1 trajectory exchange
 * The all-gather of trajectories before the update (the reference has no multi-GPU
 * path, main_train.py:109-146 runs one process) as peer-to-peer copies beside the next rollout
 * (uavhip.dist.IpcAllGather). Host-side helpers over the HIP runtime:
 *   uavhip_device_pci_id: the PCI bus id of a device of this process (>= 13 bytes): the identity
 *                         the ranks exchange, since ordinals are local to a process
 *   uavhip_device_from_pci_id: this process's ordinal of the device with that bus id (-1: not
 *                         visible here)
 *   uavhip_peer_access  : can the current device read peer_device's memory (an ordinal of THIS
 *                         process)? enables peer access (an already enabled one is fine);
 *                         *can_access = 1 for the same device
 *   uavhip_ipc_export   : IPC handle (UAVHIP_IPC_HANDLE_BYTES) of the allocation holding ptr, and
 *                         ptr's offset inside it
 *   uavhip_ipc_open     : map a peer's exported allocation into the CURRENT device's address space
 *                         (no context on the exporter's device); *ptr = base + offset
 *   uavhip_ipc_close    : unmap (the base returned by open minus its offset)
 *   uavhip_copy_async   : device-to-device copy on `stream` (a mapped peer buffer as the source) */
#define UAVHIP_IPC_HANDLE_BYTES 64
int uavhip_device_pci_id(int32_t device, char* buf, int32_t len);
int uavhip_device_from_pci_id(const char* pci_id, int32_t* device);
int uavhip_peer_access(int32_t peer_device, int32_t* can_access);
int uavhip_ipc_export(const void* ptr, void* handle, uint64_t* offset);
int uavhip_ipc_open(const void* handle, uint64_t offset, void** ptr);
int uavhip_ipc_close(void* base);
int uavhip_copy_async(void* dst, const void* src, uint64_t bytes, uavhip_stream_t stream);

/* ---------------------------------------------------------------- misc */
const char* uavhip_last_error(void);
/* 4 since round 3 (struct uavhip_ppo: the Adam hyper-parameters are doubles; the inference packed
   buffer carries split weight copies, uavhip_policy_split_layout); 5 since round 5 (the packed
   buffer ends with the range table, uavhip_policy_range_table; N > 1 peers by PCI bus id); 6: struct
   uavhip_ppo ends with `flags`, and the update step reads no environment variable any more; the
   ctypes binding refuses a library of another version */
int32_t uavhip_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* UAVHIP_H */
