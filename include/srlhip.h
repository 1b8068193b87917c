/*
 * srlhip.h — C-ABI of libsrlhip, the MI355X (gfx950) vectorised env stepper.
 *
 * Drop-in boundary for the env-step hot path of araffin/robotics-rl-srl.
 * The reference has no native ABI of its own (pure Python over the
 * third-party pybullet wheel); the seam it exposes is Python-level:
 *   - per-env gym surface      environments/srl_env.py:5-102
 *   - vec-env assembly         rl_baselines/utils.py:194-229 (createEnvs)
 *   - dataset generator loop   environments/dataset_generator.py:38-117
 * Each entry point below names the reference interface it replaces.
 * The Python host side (robotics-rl-srl_amd/srlhip) binds these with ctypes;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative SRLHIP_E* code otherwise;
 *     srlhip_last_error() gives the message (per handle; NULL handle ->
 *     thread-local message of the last failed srlhip_create).
 *   - the library owns all device memory (structure-of-arrays, one array per
 *     field, env index fastest).  Pointer arguments are borrowed for the call.
 *     cfg.io_device = 0: they are HOST pointers (the call copies and
 *     synchronises);  cfg.io_device = 1: they are DEVICE pointers on
 *     cfg.device_id and the call only enqueues work on the handle's stream
 *     (srlhip_sync() or the returned stream to order against it).
 *   - one HIP stream per handle; a handle is not thread-safe; distinct handles
 *     are independent (no global mutable state) -> one handle per GPU.
 *   - "env id" i of a handle is GLOBAL env cfg.first_env_id + i; every random
 *     stream is derived from the global id so results are invariant to how
 *     envs are sharded across GPUs (environments/utils.py:52 seeds seed+rank).
 */
#ifndef SRLHIP_H
#define SRLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRLHIP_ABI_VERSION 5   /* 2 (round 4): srlhip_kuka_tree_model grew its solver section (506 -> 510 doubles), SRLHIP_F_KUKA_BODIES;
                                 * 3 (round 5): SRLHIP_F_KUKA_IK_CROSSED;
                                 * 4 (round 6): srlhip_step_async / srlhip_step_wait / srlhip_step_pending, srlhip_config.info_bits
                                 *              (was reserved0);
                                 * 5 (round 6): srlhip_set_persistent */

/* ---- error codes ------------------------------------------------------- */
#define SRLHIP_OK            0
#define SRLHIP_EINVAL      (-22)  /* bad argument / unsupported combination     */
#define SRLHIP_ENOMEM      (-12)
#define SRLHIP_EHIP        (-5)   /* HIP runtime error (no device, launch fail) */
#define SRLHIP_ENOTSUP     (-95)  /* e.g. continuous actions on Mobile2Target   */

/* ---- env kinds: environments/registry.py:41-53 -------------------------- */
#define SRLHIP_ENV_MOBILE          0  /* MobileRobotGymEnv-v0            */
#define SRLHIP_ENV_MOBILE_1D       1  /* MobileRobot1DGymEnv-v0          */
#define SRLHIP_ENV_MOBILE_2TARGET  2  /* MobileRobot2TargetGymEnv-v0     */
#define SRLHIP_ENV_MOBILE_LINE     3  /* MobileRobotLineTargetGymEnv-v0  */
#define SRLHIP_ENV_KUKA_BUTTON     4  /* KukaButtonGymEnv-v0             */
#define SRLHIP_ENV_KUKA_MOVING     5  /* KukaMovingButtonGymEnv-v0 (kuka_moving_button_gym_env.py) */
#define SRLHIP_ENV_KUKA_2BUTTON    6  /* Kuka2ButtonGymEnv-v0 (kuka_2button_gym_env.py): two buttons pressed in order */
#define SRLHIP_ENV_KUKA_RAND       7  /* KukaRandButtonGymEnv-v0 (kuka_rand_button_gym_env.py:59-71,111-125): the ten dropped objects and the kicked ball are
                                        * free bodies the arm can push (full model: proxy shapes, table contact + friction, arm-sphere contacts —
                                        * srlhip_get_state KUKA_BODIES); scenery at rest with the lumped model */
#define SRLHIP_ENV_LAST            SRLHIP_ENV_KUKA_RAND

/* ---- observation modes: kuka_button_gym_env.py:162-173 ------------------ */
#define SRLHIP_OBS_GROUND_TRUTH     0  /* f32[obs_dim] relative position        */
#define SRLHIP_OBS_JOINTS           1  /* Kuka only: 14 constant joint values   */
#define SRLHIP_OBS_JOINTS_POSITION  2  /* Kuka only: 3 + 14                      */
#define SRLHIP_OBS_RAW_PIXELS       3  /* u8[H,W,3(6)] from the tile rasteriser  */

/* ---- Kuka body model: what loadSDF("kuka_iiwa/kuka_with_gripper2.sdf") (kuka.py:60) becomes ------------------
 * FULL   : the 12-DoF tree — arm J0..J6, gripper_to_arm, two fingers, two finger tips — every joint driven by the
 *          POSITION_CONTROL motor the reference commands each step (kuka.py:167-187: arm 200 N·m / 0.35 rad/s, joint 7
 *          200, fingers 2 / 2.5, tips 2), contact spheres on links 5..11, one friction row per contact.  Stepped by the
 *          tree lane-group kernel (csrc/kuka_tree.hpp) at every batch size.  The default of every Kuka env
 *          (Kuka2ButtonGymEnv: the kernel's two-button form — second glider, its motor / stop rows, its cap and base).
 * LUMPED : rounds 1-2 — the gripper welded to link_7 (7 DoF), six gripper spheres, frictionless contacts.  Kept as the
 *          cheaper approximation (profiles/r03_kuka_model_gap.json measures what it costs: 0.02 rad on the arm joints,
 *          different reward / done planes). */
#define SRLHIP_KUKA_MODEL_LUMPED 0
#define SRLHIP_KUKA_MODEL_FULL   1

/* ---- random-number modes ------------------------------------------------- */
#define SRLHIP_RNG_HOST     0  /* caller supplies every random draw (parity harness)        */
#define SRLHIP_RNG_PHILOX   1  /* device Philox4x32-10 keyed (seed, global env id): throughput */
#define SRLHIP_RNG_MT19937  2  /* device-resident numpy RandomState per env: reproduces the
                                  reference's env.np_random stream (srl_env.py:71-78)       */

typedef struct srlhip_env *srlhip_handle;

typedef struct srlhip_config {
    int32_t struct_size;      /* = sizeof(srlhip_config), ABI check                        */
    int32_t env_kind;         /* SRLHIP_ENV_*                                              */
    int32_t num_envs;         /* envs owned by this handle (this GPU's shard)              */
    int32_t device_id;        /* HIP device ordinal                                        */
    int32_t first_env_id;     /* global id of env 0 (sharding offset)                      */
    int32_t is_discrete;      /* ctor kwarg is_discrete   (mobile_robot_env.py:61)         */
    int32_t random_target;    /* ctor kwarg random_target                                  */
    int32_t force_down;       /* ctor kwarg force_down    (Kuka)                           */
    int32_t shape_reward;     /* ctor kwarg shape_reward                                   */
    int32_t action_repeat;    /* ctor kwarg action_repeat (Kuka, >=1)                      */
    int32_t action_joints;    /* ctor kwarg action_joints (Kuka)                           */
    int32_t obs_mode;         /* SRLHIP_OBS_*  (ctor kwarg srl_model)                      */
    int32_t img_h, img_w;     /* raw_pixels size (reference: 224x224)                      */
    int32_t multi_view;       /* second camera stacked behind the first (6-channel image): ctor kwarg
                                 multi_view (Kuka, kuka_button_gym_env.py:401-417) / fpv (MobileRobot,
                                 mobile_robot_env.py:313-332: the camera riding on the robot)       */
    int32_t rng_mode;         /* SRLHIP_RNG_*                                              */
    int32_t auto_reset;       /* 1: step() resets finished envs itself and returns the first
                                 observation of the next episode (SB VecEnv semantics,
                                 rl_baselines/utils.py:216-220); needs rng_mode != HOST     */
    int32_t io_device;        /* 0 host pointers, 1 device pointers (see Conventions)      */
    int32_t kuka_model;       /* SRLHIP_KUKA_MODEL_* (Kuka envs; srlhip_default_config picks FULL where it exists) */
    int32_t info_bits;        /* 0: done_out bytes are 0 / 1.  1 (full-model Kuka handles; ignored elsewhere): bit 1 of every
                                 done_out byte = the env-step ran under the IK conditioning flag (SRLHIP_F_KUKA_IK_CROSSED bit 0,
                                 sampled BEFORE an auto-reset clears it) — the per-step `infos` of the VecEnv surface    */
    int64_t seed0;            /* base seed: env i is seeded seed0 + first_env_id + i       */
    double  max_distance;     /* ctor kwarg max_distance                                   */
} srlhip_config;

/* Fill *cfg with the reference's ctor defaults for env_kind
 * (kuka_button_gym_env.py:78-81, mobile_robot_env.py:61-64). */
int srlhip_default_config(int32_t env_kind, srlhip_config *cfg);

/* Replaces: env construction in makeEnv/_make (environments/utils.py:36-95),
 * one call for the whole batch instead of one process per env. Seeds every env
 * with seed0 + global id, but does not reset. */
int srlhip_create(const srlhip_config *cfg, srlhip_handle *out);
int srlhip_destroy(srlhip_handle h);

/* Shapes implied by the config (observation_space / action_space of the env). */
int srlhip_obs_dim(srlhip_handle h);          /* floats per env (ground truth modes)   */
int srlhip_obs_bytes(srlhip_handle h);        /* bytes per env of one observation      */
int srlhip_action_dim(srlhip_handle h);       /* 1 (discrete) | 2 | 3 | 7              */
int srlhip_num_actions(srlhip_handle h);      /* Discrete(n): n ; 0 if continuous      */

/* Replaces SRLGymEnv.seed (srl_env.py:71-78) for the envs selected by mask
 * (NULL = all).  seeds[i] is the integer the reference would pass to
 * env.seed(); MT19937 mode hashes it exactly like gym (sha512 -> init_by_array).
 * mask/seeds are always HOST pointers. */
int srlhip_seed(srlhip_handle h, const uint8_t *mask, const int64_t *seeds);

/* Replaces <Env>.reset() (mobile_robot_env.py:159-222, kuka_button_gym_env.py:214-281)
 * for the envs selected by mask (NULL = all; HOST pointer).
 * host_rand: RNG_HOST only — [num_envs][srlhip_reset_rand_count()] doubles, the
 *            values the reference's np_random calls would return, in draw order.
 * obs_out:   [num_envs][obs] — rows of unselected envs are left untouched. */
int srlhip_reset(srlhip_handle h, const uint8_t *mask, const double *host_rand, void *obs_out);
int srlhip_reset_rand_count(srlhip_handle h);

/* Replaces VecEnv.step / <Env>.step (mobile_robot_env.py:235-280,
 * kuka_button_gym_env.py:293-368) for the whole batch.
 * actions: discrete -> int32[num_envs], value -1 == the reference's `None`
 *          action (kuka_button_gym_env.py:295-299);  continuous -> float[num_envs][adim].  On a Kuka handle a
 *          continuous row whose every component is NaN is that same `None` (no noise draw; Cartesian mode: zero
 *          increment, joint mode: targets held at the initial joint positions).  Host-pointer calls return SRLHIP_EINVAL
 *          for every other non-finite value (a partly NaN row, an infinity) and for any NaN on a MobileRobot handle
 *          (whose reference step has no continuous `None`); device-pointer calls own their buffers, and there the
 *          kernels look at component 0 only.
 * host_noise: RNG_HOST only — double[num_envs], value of np_random.normal(...) per env.
 * obs_out [num_envs][obs], reward_out float[num_envs], done_out uint8[num_envs].
 * With cfg.auto_reset the observation of a finished env is the first one of its
 * next episode. */
int srlhip_step(srlhip_handle h, const void *actions, const double *host_noise,
                void *obs_out, float *reward_out, uint8_t *done_out);

/* srlhip_step in two halves, for HOST-pointer handles (cfg.io_device = 0): what SubprocVecEnv.step_async / step_wait are to the
 * reference (rl_baselines/utils.py:213-220 builds the SubprocVecEnv whose step_async only SENDS the actions to the workers and whose
 * step_wait collects them).  srlhip_step_async validates the inputs, copies them into the handle's pinned block and ENQUEUES the
 * step on the handle's stream: it returns before the GPU has run it, so a caller holding G handles (one per GPU — the sharded
 * HipVecEnv) has all G devices stepping at once, and a single-handle caller overlaps its own work with the step.
 * srlhip_step_wait waits for that step and copies its planes out (any pointer may be NULL); with cfg.auto_reset the observation of
 * a finished env is the first one of its next episode.  One step may be pending per handle: a second srlhip_step_async, or a
 * srlhip_step, before the wait returns SRLHIP_EINVAL; srlhip_step_wait without a pending step too.  srlhip_step ==
 * srlhip_step_async + srlhip_step_wait.  srlhip_step_pending: 1 between the two, else 0. */
int srlhip_step_async(srlhip_handle h, const void *actions, const double *host_noise);
int srlhip_step_wait(srlhip_handle h, void *obs_out, float *reward_out, uint8_t *done_out);
int srlhip_step_pending(srlhip_handle h);
/* (Zero-copy steps of the full-model Kuka kernels and of the MobileRobot family do not wait for the kernel's END: the kernel reports the step's outputs per
 * eighth of its grid — one XCD each, checked per launch — after one L2 write-back, and srlhip_step / srlhip_step_wait poll
 * those words; the stream synchronisation remains the fallback.  SRLHIP_STEP_SIGNAL=0 switches the signal off.  What the call
 * returns — observations, rewards, dones, Monitor's records — is complete; the kernel's exit stores of the STATE planes may still be
 * in flight on the handle's stream: every entry point of this library is ordered behind them, a caller that reads
 * srlhip_device_ptr() planes of a host-pointer handle from a stream of its own calls srlhip_sync() first.) */

/* Persistent stepping (opt-in; host-pointer handles of the MobileRobot family, KukaButtonGymEnv, KukaMovingButtonGymEnv and
 * Kuka2ButtonGymEnv — any action mode and any observation mode but raw pixels — on a device RNG mode, whose wavefronts are all resident at once: up to
 * 4096 envs on an MI355X; SRLHIP_ENOTSUP otherwise): the step pair WITHOUT a kernel launch per step.  One launch of the rollout kernel stays on
 * the device with every env's state in registers.  srlhip_step_async writes the actions and a sequence number into mapped
 * memory; workgroup 0 polls that word over PCIe and relays it through device memory; every wavefront has already run everything
 * in front of the action (dynamics, collision detection, on a contact step the solver's setup) while it waited, finishes the step and writes its
 * outputs to the host's mapped planes with plain stores — they stay in its XCD's L2; the last wavefront of each eighth of the
 * grid (= one XCD, verified at launch through HW_REG_XCC_ID) to finish writes that L2 back with ONE system-scope release and
 * writes the eighth's `done` word; srlhip_step_wait polls those 8 words.  (Where an eighth does not sit on one XCD, or with
 * SRLHIP_PERSIST_STAGED=1, the outputs go through a staging copy in device memory that the eighth's last wavefront copies out.)  What a per-step launch pays every time — the launch itself, the
 * 5.6 KB model table, ~40 state planes, the generators, forward kinematics, the stream synchronisation — is paid once: measured
 * HipVecEnv.step 82 -> 62 us at 4096 envs, 61 -> 44 at 256, 39 -> 28 at 16 (launching path -> persistent; MobileRobot: 19 -> 13 us
 * and 13 -> 6 us at 16 envs).  Same kernel
 * code, same arithmetic: results are those of the launching path bit for bit (tests/test_gpu_persistent_step.py).
 * The kernel PARKS (writes the state back and exits) when any other entry point touches the handle, and by itself when no step
 * arrived for park_us microseconds (<= 0: 2000) — the next step restarts it, at the cost of a launch.  While it is resident it
 * holds one wavefront slot and 40 KB of LDS on every SIMD it uses (all of them at 4096 envs): use it when the policy runs on
 * the host or on another device (a random agent, ARS / CMA-ES with a numpy policy, a policy server) and answers within park_us.
 * A workgroup that could not become resident shows up as a step that never completes: srlhip_step_wait then parks the kernel
 * and fails with SRLHIP_EHIP after ~20 s instead of hanging.  on = 0 switches back to launches.  The actions are those of
 * srlhip_step: -1, or a continuous row of NaNs, is `None` (the part of the step run before the action holds for it too). */
int srlhip_set_persistent(srlhip_handle h, int32_t on, int32_t park_us);

/* Fused rollout: T consecutive steps with auto-reset, outputs streamed as
 * [T][num_envs] planes.  Replaces the random-agent hot loop
 * (rl_baselines/random_agent.py:35-42, dataset_generator.py:91-105).
 * actions_TN: int32/float [T][num_envs]([adim]) or NULL -> uniform random
 * actions drawn on the device (returned in act_out_TN if not NULL).  `None` rows as in srlhip_step
 * (-1; on a Kuka handle with continuous actions a row of NaNs), checked the same way on host pointers.
 * Requires cfg.auto_reset and rng_mode != HOST.  Any output may be NULL. */
int srlhip_rollout(srlhip_handle h, int32_t T, const void *actions_TN,
                   void *obs_TN, float *reward_TN, uint8_t *done_TN, void *act_out_TN);

/* Fused rollout of a per-env LINEAR POLICY (the ARS policy, rl_baselines/evolution_strategies/ars.py): like srlhip_rollout, but
 * the action of every step is chosen inside the kernel from the env's current float32 observation o (at the first step the
 * observation of the state the call found, afterwards the one the previous step produced — after an auto-reset the new episode's
 * first one):  score_a = sum_d (double)x_d * W[d][a] in float64, d ascending, x = o or its frozen VecNormalize image;
 * discrete actions: a = argmax, lowest index wins a tie; continuous actions: the row (float)score_a, not clipped.
 * (A score that is zero carries the IEEE sign of that sum: -0.0 where every product x_d * W[d][a] is -0.0, else +0.0.)
 * Everything behind the action is srlhip_rollout's step.  act_out_TN receives the actions taken (the `None` rows of frozen envs
 * included); any output may be NULL.
 * Needs cfg.auto_reset, a device RNG mode, ground-truth observations and a MobileRobot env, KukaButtonGymEnv, KukaMovingButtonGymEnv
 * or Kuka2ButtonGymEnv on the full model (any action mode the env has); everything else — the joints / joints_position observation
 * modes, raw pixels, KukaRandButtonGymEnv, the lumped model, RNG_HOST — returns SRLHIP_ENOTSUP with a message naming it.  Host-pointer handles: EINVAL for non-finite weights / mean
 * and for std entries that are not finite and > 0.  EINVAL while a srlhip_step_async is pending.  A resident kernel parks.
 * Capturable under srlhip_graph_begin on device-pointer handles. */
typedef struct srlhip_linear_policy {
    int32_t struct_size;        /* sizeof(srlhip_linear_policy): ABI check */
    int32_t per_env;            /* 1: weights [num_envs][obs_dim][A]; 0: one [obs_dim][A] for every env (A = num_actions or action_dim) */
    int32_t freeze_after_done;  /* 1: from the step AFTER an env's first done in this call it takes the `None` action
                                   (-1; Kuka continuous: a row of NaNs; MobileRobot continuous: a zero row) for the rest of the call */
    int32_t normalize;          /* 1: x_d = (float) clamp(((double)o_d - mean[d]) / std[d], -clip_obs, clip_obs) first */
    const double *weights, *obs_mean, *obs_std;   /* follow cfg.io_device like every other pointer; mean / std: [obs_dim] */
    double clip_obs;
} srlhip_linear_policy;
int srlhip_rollout_policy(srlhip_handle h, int32_t T, const srlhip_linear_policy *pol,
                          void *obs_TN, float *reward_TN, uint8_t *done_TN, void *act_out_TN);

/* Fused rollout of a per-env ONE-HIDDEN-LAYER ReLU MLP POLICY (the CMA-ES policy, rl_baselines/evolution_strategies/cma_es.py:
 * MLPPolicyPytorch(obs_dim, [H], A)): srlhip_rollout_policy with another score function.  params holds, per env (per_env) or once,
 * P = H*D + H + A*H + A float32 values in nn.Module.parameters() order — fc_in.weight [H][D], fc_in.bias [H], fc_out.weight [A][H],
 * fc_out.bias [A] (D = obs_dim, A = num_actions or action_dim) — the layout of a CMA-ES candidate vector, so a [num_envs][P]
 * population is passed as it is.  With x the float32 observation or its frozen VecNormalize image, formed exactly as in
 * srlhip_rollout_policy:
 *     h_j = max(0, b1_j + sum_d W1[j][d] * x_d),   score_a = b2_a + sum_j W2[a][j] * h_j,
 * every product and sum in float64 (the float32 parameters and x converted first; a product and the sum that takes it may be one
 * fused multiply-add).  The ORDER of the sum over j is the kernel's: a group of 16 lanes works on one env, lane l sums its units
 * l, l+16, ... in that order and the 16 partial sums are then reduced in a fixed pattern — so scores agree with any other summation
 * order only to float64 rounding (|error| <= 2^-46 * (|b2_a| + sum_j |W2[a][j]| * (|b1_j| + sum_d |W1[j][d] * x_d|)) for H <= 128),
 * but the order is FIXED: two calls on equal state and parameters give equal bits.
 * Fifteen of the sixteen partial sums start from +0.0 (fc_out's bias sits with lane 0), so a score that is zero is +0.0 whatever the
 * signs of b2_a and of the zero products.
 * Action selection (strict argmax, lowest index first / the row (float)score_a), freeze_after_done, auto-reset, NULL output planes,
 * chunked calls, graph capture and the parked resident kernel are srlhip_rollout_policy's, and so is the set of refusals
 * (SRLHIP_ENOTSUP naming the cause: joints / joints_position / raw_pixels observations, KukaRandButtonGymEnv, the lumped model,
 * RNG_HOST, no auto_reset), plus Kuka2ButtonGymEnv with joint-space continuous actions (the env takes discrete actions in the
 * reference; its kernels have six score rows, not seven).  EINVAL: hidden outside 1..128, reserved != 0, a wrong struct_size, a pending srlhip_step_async and, on
 * host-pointer handles, non-finite params / mean or std entries that are not finite and > 0. */
typedef struct srlhip_mlp_policy {
    int32_t struct_size;        /* sizeof(srlhip_mlp_policy): ABI check */
    int32_t per_env;            /* 1: params [num_envs][P]; 0: one [P] for every env */
    int32_t freeze_after_done, normalize;   /* as in srlhip_linear_policy */
    int32_t hidden;             /* H, 1..128 (the reference uses 100) */
    int32_t reserved;           /* 0 */
    const float *params;        /* follows cfg.io_device like every other pointer */
    const double *obs_mean, *obs_std;       /* [obs_dim] */
    double clip_obs;
} srlhip_mlp_policy;
int srlhip_rollout_mlp_policy(srlhip_handle h, int32_t T, const srlhip_mlp_policy *pol,
                              void *obs_TN, float *reward_TN, uint8_t *done_TN, void *act_out_TN);

/* srlhip_rollout_mlp_policy with another action selection: the discrete action is DRAWN from the softmax of the scores, as CMA-ES does
 * without --deterministic (rl_baselines/evolution_strategies/cma_es.py: np.random.choice(len(a), p=softmax(scores))).  Discrete action
 * modes only.  The scores score_0 .. score_{A-1} are formed exactly as above.  At step t of the call (t = 0 .. T-1), for env e whose
 * action-stream counter was c0 when the call began:
 *     u   = Philox::to_double(o[0], o[1]) of the Philox4x32-10 block at counter c0 + t, stream 1, key of env e (its seed): the
 *           generator's double01(), so u lies in [0, 1);
 *     m   = max_k score_k;
 *     w_k = exp(score_k - m) in float64, through the device math library;
 *     c_k = w_0 + ... + w_k, added in index order;
 *     z   = u * c_{A-1};
 *     a   = the number of k < A-1 with z >= c_k      (the inverse CDF, branch-free: the last index takes whatever rounding leaves).
 * An env frozen by freeze_after_done takes -1 as above; its draw at c0 + t is discarded, not skipped.  After the call the counter is
 * c0 + T for every env, whatever happened in between: chunked calls equal one call, and the draws are random-access.
 * The stream is the one srlhip_rollout(actions = NULL) draws the synthetic agent's actions from (one counter per env, reset to 0 by
 * srlhip_seed), so a sampled rollout continues where that left off and the reverse.  What that call adds to the counter per step:
 * MobileRobot family, discrete actions: 1 — but there the counter counts ACTIONS, four to a block (action i is word i % 4 of block
 * i / 4), while this call reads the counter as a BLOCK index: after 40 synthetic steps from 0 the sampled call starts at block 40, and
 * after T sampled steps the synthetic agent goes on at action c0 + T; MobileRobot continuous: 1 block; Kuka envs, discrete: 1 block;
 * Kuka continuous: (action_dim + 1) / 2 blocks (2, or 4 in the joint-space mode).
 * The draw does not depend on cfg.rng_mode: an MT19937 handle keeps the reference's np_random stream for the env and uses this Philox
 * stream for the actions — the split the synthetic agent already has.
 * The bits are fixed for a given build of this library.  exp is the device library's, so against another implementation of the
 * contract the action is pinned only where z is not within the rounding of the c_k (tests/mlp_sample_ref.py: with the score bound
 * above, E = 2 max_k tol_k and rho = expm1(E) + 2^-48, an action a is accepted iff (a == 0 or z (1 + rho) >= c_{a-1} (1 - rho)) and
 * (a == A-1 or z (1 - rho) < c_a (1 + rho))).
 * Refusals: everything srlhip_rollout_mlp_policy refuses, worded alike under the prefix "rollout_mlp_policy_sampled:", and
 * SRLHIP_ENOTSUP for the continuous action modes (the message names "discrete": the reference never samples continuous actions).
 * EINVAL cases, graph capture on device-pointer handles, NULL planes and the parking of a resident kernel are as above. */
int srlhip_rollout_mlp_policy_sampled(srlhip_handle h, int32_t T, const srlhip_mlp_policy *pol,
                                      void *obs_TN, float *reward_TN, uint8_t *done_TN, void *act_out_TN);

/* srlhip_rollout_policy with the selection of srlhip_rollout_mlp_policy_sampled: the discrete action is DRAWN from the softmax of the
 * linear policy's scores, as ARS does without --deterministic (rl_baselines/evolution_strategies/ars.py: np.random.choice(len(a),
 * p=softmax(obs @ (M +- nu delta_k)))).  Discrete action modes only.  The struct is srlhip_linear_policy, unchanged.
 *   scores     srlhip_rollout_policy's: score_a = sum_d (double)x_d * W[d][a], d ascending, starting with the d = 0 product — the
 *              MobileRobot kernels in exactly this order with no product fused (the arithmetic of srlhip_policy_act's linear form, bit
 *              for bit), the Kuka kernels with the freedom to fuse a product with the sum that takes it.
 *   selection  the draw of srlhip_rollout_mlp_policy_sampled word for word (u, m, w_k, c_k, z, a): u from the Philox block at counter
 *              c0 + t, stream 1, key of env e; an env frozen by freeze_after_done takes -1 and its draw is discarded, not skipped.
 * After the call the action-stream counter is c0 + T for every env: chunked calls equal one call.  The stream, what srlhip_rollout(actions
 * = NULL) adds to its counter per step (MobileRobot, discrete: the counter is read here as a BLOCK index), and the independence of
 * cfg.rng_mode are as described there.  One step of this call equals srlhip_policy_act(linear, score_out) followed by
 * srlhip_sample_actions on a MobileRobot handle, bit for bit.
 * Against another implementation of the contract the action is pinned only where z is not within the rounding of the c_k
 * (tests/policy_sample_ref.py: the acceptance rule above with the score bound (2 D + 16) 2^-53 sum_d |x_d W[d][a]|).
 * Refusals: everything srlhip_rollout_policy refuses, worded alike under the prefix "rollout_policy_sampled:", and SRLHIP_ENOTSUP for
 * the continuous action modes (the message names "discrete").  EINVAL cases, graph capture on device-pointer handles, NULL planes and
 * the parking of a resident kernel are srlhip_rollout_policy's. */
int srlhip_rollout_policy_sampled(srlhip_handle h, int32_t T, const srlhip_linear_policy *pol,
                                  void *obs_TN, float *reward_TN, uint8_t *done_TN, void *act_out_TN);

/* The four fused policy rollouts with the REDUCED result a learner keeps instead of the [T][num_envs] planes: per env the return up
 * to its first done, the number of live steps and the first two moments of the live observations (what ARS, CMA-ES and
 * DeviceVecNormalize otherwise form from the planes with a chain of reductions).  No plane is allocated or written.
 * Exactly one of `linear` / `mlp` is non-null (as in srlhip_policy_act); sample != 0 selects the _sampled form of that policy.  The
 * pointers of `out` follow cfg.io_device like every other pointer.
 * THE CALL IS THE PLANE CALL WITH OTHER OUTPUTS: stepping, action selection, RNG consumption, action-stream counters, auto-resets,
 * freeze_after_done and episode statistics are those of the corresponding plane call (srlhip_rollout_policy, srlhip_rollout_mlp_policy
 * or their _sampled forms) with the same arguments; the env state after the call equals the plane call's bit for bit.  In terms of
 * the rows reward[t][e], done[t][e] and o[t][e][d] (the raw float32 observation) that plane call would have written:
 *   first(e)       the first row t of THIS call at which env e reports done (bit 0 of the done byte); T if there is none
 *   ret[e]         sum over t < first(e) of (double)reward[t][e], added in ascending t from +0.0; the reporting step is not counted
 *   length[e]      min(first(e) + 1, T)
 *   obs_sum[e][d]  sum over t < length(e) of (double)o[t][e][d], ascending t from +0.0
 *   obs_sqsum[e][d] the same sum of (double)o * (double)o: each product is rounded, then added (never fused with the sum) — a
 *                  sequential float64 loop over the planes reproduces every output bit for bit (tests/rollout_summary_ref.py)
 * PER-CALL SCOPE: the result depends on T and on nothing earlier — an episode that was running when the call began counts from the
 * call's first row, and the result of two calls of T/2 steps is NOT the result of one call of T steps (first(e) restarts with every
 * call).  It does not compose across chunked calls.
 * Refusals: everything the corresponding plane call refuses, worded alike under the prefix "rollout_policy_summary:" (the
 * discrete-only rule of `sample` and Kuka2Button's missing joint-space arm included).  SRLHIP_EINVAL: both or neither policy, a null
 * `out` or out->ret, only one of the two moment pointers, a wrong struct_size (of `out` or of the policy), reserved != 0, T <= 0, a
 * pending srlhip_step_async, the plane calls' pointer checks and, on host-pointer handles, their value checks.  A resident persistent
 * kernel parks.  One launch on the handle's stream (Kuka: and the header kernel); on device-pointer handles no allocation and no
 * synchronisation: capturable under srlhip_graph_begin. */
typedef struct srlhip_rollout_summary {
    int32_t struct_size, reserved;      /* sizeof(srlhip_rollout_summary), 0 */
    double  *ret;                       /* [num_envs]            required */
    int32_t *length;                    /* [num_envs]            or NULL  */
    double  *obs_sum, *obs_sqsum;       /* [num_envs][obs_dim]   both or neither */
} srlhip_rollout_summary;
int srlhip_rollout_policy_summary(srlhip_handle h, int32_t T, const srlhip_linear_policy *linear, const srlhip_mlp_policy *mlp,
                                  int32_t sample, const srlhip_rollout_summary *out);

/* The policy's action as a call of its own: ONE step of the three fused rollouts' action selection, from an observation plane the
 * caller already holds on the device — the state vectors an SRL encoder made of the rendered frames (image -> encoder -> state ->
 * policy), where no policy can sit inside the physics kernel.  A T-step rollout on learned states is T x (srlhip_policy_act,
 * srlhip_step, srlhip_encoder_forward), every call enqueue-only on the handle's stream, no host read in the loop.
 * Exactly one of `linear` / `mlp` is non-null; the structs are the fused rollouts', unchanged, with obs_dim (D, 1..1024) in the place of
 * the handle's own observation size (weights [D][A], params P = H D + H + A H + A, obs_mean / obs_std [D]; A = num_actions or
 * action_dim of the handle).  Device-pointer handles only (cfg.io_device = 1; SRLHIP_ENOTSUP otherwise), ANY env kind, model and
 * observation mode, raw pixels included: the call reads the handle's action space and its action-stream counters, never the env state.
 *   obs        float32 [num_envs][D]
 *   done_prev  uint8 [num_envs], the done plane of the step that produced obs, or NULL at the first step of a rollout; only bit 0 counts
 *              (bit 1 is cfg.info_bits')
 *   frozen     uint8 [num_envs], read and written when pol.freeze_after_done (required then): first frozen |= done_prev & 1, then a
 *              frozen env takes the `None` action of srlhip_linear_policy.freeze_after_done (-1; Kuka continuous: a row of NaNs, bits
 *              0x7fc00000; MobileRobot continuous: a zero row).  The caller zeroes the plane at the start of a rollout.  Without
 *              freeze_after_done neither plane is read or written.
 *   act_out    int32 [num_envs] or float32 [num_envs][A]: the row the caller wants written, e.g. row t of a [T][num_envs] plane.
 *   score_out  NULL, or float64 [num_envs][A]: the scores as they stood in front of the selection (frozen envs included) — what the
 *              tests compare bit for bit; a rollout passes NULL.
 * ARITHMETIC, order-exact (csrc/policy_act.hpp is its one text for device and host, built with -ffp-contract=off: no product is fused
 * with the sum that takes it; tests/policy_act_ref.py restates it in numpy bit for bit):
 *   x_d      = o_d, or with normalize (float) min(max(((double)o_d - mean[d]) / std[d], -clip_obs), clip_obs)
 *   linear   score_a = (double)x_0 W[0][a] + (double)x_1 W[1][a] + ..., d ascending in float64; the sum starts with the d = 0 product
 *   MLP      pre_j = (double)b1_j + (double)W1[j][0] (double)x_0 + ..., d ascending; h_j = pre_j > 0 ? pre_j : +0.0.
 *            A virtual row of 16 lanes: lane l owns the units l, l + 16, ... < H; its partial p_l starts from (double)b2_a (lane 0) or
 *            +0.0 (lanes 1..15) and takes (double)W2[a][j] h_j for its units in ascending order.  The sixteen partials are combined in
 *            four stages, in each of which every lane adds its partner's value to its own: partner l ^ 1, then l ^ 2, then 7 - l inside
 *            each half of eight lanes, then 15 - l; score_a is what lane 0 then holds (every lane holds the same bits).
 *   These are the sums of srlhip_rollout_policy / srlhip_rollout_mlp_policy with the freedom taken out: the fused MobileRobot kernels
 *   compute exactly this, the fused Kuka kernels may fuse a product with its sum.  Against any other float64 summation of the same
 *   terms: |difference| <= (2 D + H + 16) 2^-53 S_a,  S_a = |b2_a| + sum_j |W2[a][j]| (|b1_j| + sum_d |W1[j][d] x_d|) — a chain of D + 1
 *   roundings per unit and at most 13 behind it on this side, at most D + H + 2 on the other, to first order.  (The 2^-46 of
 *   srlhip_rollout_mlp_policy is this figure at H = 128 and the D <= 3 of a ground-truth observation; at D = 1024 it is 2^-41.9.)
 *   selection  discrete: the strict argmax, lowest index first; continuous: the row (float)score_a; sample != 0 (MLP and discrete action
 *            modes only): the inverse-CDF draw of srlhip_rollout_mlp_policy_sampled word for word (m, w_k, c_k, z, a; exp from the
 *            device math library), with u from the Philox block at the env's CURRENT action-stream counter c, stream 1.
 * COUNTER: a sampled call leaves c + 1 for EVERY env, frozen or not, and advances it inside the kernel — a captured call draws fresh
 * numbers at every replay.  One srlhip_policy_act(sample) equals one step of srlhip_rollout_mlp_policy_sampled: K calls from c0 use
 * the blocks c0 .. c0 + K - 1 that one fused call with T = K uses, and leave c0 + K as it does; the counter is the one
 * srlhip_rollout(actions = NULL) draws from (what that call adds per step: see above).  As there, the draw does not depend on cfg.rng_mode.
 * A non-sampled call does not touch the counter.
 * The result for env e depends on its own row of obs, its parameters, done_prev[e], frozen[e] and its counter alone: not on num_envs,
 * on e, or on the launch geometry — shards and batch sizes agree bit for bit.
 * One launch on the handle's stream, no allocation, no synchronisation; capturable under srlhip_graph_begin.  Every parameter block is
 * read once (a shared block: once per workgroup of four envs).  SRLHIP_EINVAL: both or neither policy, a wrong struct_size, hidden
 * outside 1..128, reserved != 0, obs_dim outside 1..1024, sample with a linear policy, a null obs / act_out / parameter block, normalize
 * without mean and std, freeze_after_done without the frozen plane, a pending srlhip_step_async.  SRLHIP_ENOTSUP: a host-pointer
 * handle; sample on a continuous action mode (the message names "discrete").  A resident persistent kernel parks. */
int srlhip_policy_act(srlhip_handle h, const srlhip_linear_policy *linear, const srlhip_mlp_policy *mlp, int32_t sample,
                      const float *obs, int32_t obs_dim, const uint8_t *done_prev, uint8_t *frozen, void *act_out, double *score_out);

/* The policy's action FROM THE FRAME: srlhip_policy_act for the reference's CNN-from-pixels policy (CMA-ES with --srl-model raw_pixels,
 * rl_baselines/evolution_strategies/cma_es.py: CNNPolicyPytorch), every env with its own network.  A T-step rollout from pixels is
 * T x (srlhip_cnn_policy_act, srlhip_step), every call enqueue-only on the handle's stream, no host read in the loop.
 * Device-pointer handles only (cfg.io_device = 1; SRLHIP_ENOTSUP otherwise), cfg.obs_mode = raw pixels (SRLHIP_ENOTSUP otherwise), any env
 * kind and model: the call reads the handle's frame shape, action space and action-stream counters, never the env state.
 *   images     uint8 [num_envs][H][W][C], the plane srlhip_step / srlhip_reset write: H = cfg.img_h, W = cfg.img_w, C = 3, or 6 with
 *              cfg.multi_view.  Every side from 43 to 224 (SRLHIP_ENOTSUP outside: below 43 the third pooled plane is empty).
 *   params     float32 [num_envs][P] (per_env) or [P], in nn.Module.parameters() order — the layout of a CMA-ES candidate vector:
 *              conv1.weight [8][C][5][5], norm1.weight [8], norm1.bias [8], conv2.weight [16][8][3][3], norm2.weight [16], norm2.bias [16],
 *              conv3.weight [32][16][3][3], norm3.weight [32], norm3.bias [32], fc.weight [A][F], fc.bias [A]; A = num_actions or
 *              action_dim of the handle, F = 32 h3 w3 with h3 x w3 the plane behind the third pool (224 x 224: F = 288 as in the
 *              reference, P = 8206 at C = 3, A = 6; other sizes: the linear layer the reference would need there).
 *   done_prev, frozen, act_out: as in srlhip_policy_act (the `None` rows of frozen envs included).
 *   score_out  NULL, or float32 [num_envs][A]: the scores as they stood in front of the selection (frozen envs included).
 * NETWORK.  x = (float)(byte / 255.0), NHWC read as NCHW.  Three times: a convolution without bias, stride 2 (5x5 pad 2 to 8 channels,
 * 3x3 pad 1 to 16, 3x3 pad 1 to 32; plane side (s + 2 pad - k) / 2 + 1), batch-norm, ReLU, max-pool 2x2 (floor).  The batch-norm is
 * the reference's as it RUNS: never put in eval mode, one observation per forward, so the statistics are this frame's own per-channel
 * mean and biased variance over the whole conv plane (before the pool), eps = 1e-5; gamma and beta are parameters, running statistics play
 * no part.  Then the pooled planes flattened channel-major and score_a = fc.bias[a] + sum_f fc.weight[a][f] x_f.
 * ARITHMETIC (csrc/cnn_policy.hpp is its one text for device and host, built with -ffp-contract=off on both sides, so the device's scores
 * equal the host program's bit for bit): conv sums in float32, taps in (input channel, row, column) order from +0; a channel's sum and sum
 * of squares in float64 (partial sums per thread of the workgroup, a fixed pairwise tree over them); mean = S / n, var = max(Q / n - mean^2, 0),
 * g = gamma / sqrt(var + eps) in float64; y = max((float)(((double)x - mean) g + beta), 0).  The pool is taken BEFORE the normalisation —
 * the window's max where gamma >= 0, its min where gamma < 0: y is monotone in x in that direction, rounding included, so this is the
 * pooled value of the normalised plane itself.  The linear layer: float64 from (double)bias, f ascending, rounded to float32 once.
 * Against the float64 forward the scores agree to float32 rounding of the conv sums (tests/cnn_policy_ref.py has the measured figures).
 *   selection  on (double)score_a, the functions of srlhip_policy_act (csrc/policy_act.hpp): discrete: the strict argmax, lowest index
 *            first; continuous: the row score_a; sample != 0 (discrete action modes only): the inverse-CDF draw of
 *            srlhip_rollout_mlp_policy_sampled word for word, with u from the Philox block at the env's CURRENT action-stream counter c, stream 1.
 * COUNTER: a sampled call leaves c + 1 for EVERY env, frozen or not, and advances it inside the kernel — a captured call draws fresh
 * numbers at every replay; K calls from c0 use the blocks c0 .. c0 + K - 1 that srlhip_rollout_mlp_policy_sampled with T = K uses.
 * A non-sampled call does not touch the counter.
 * The result for env e depends on its own frame, its parameters, done_prev[e], frozen[e] and its counter alone: not on num_envs, on e,
 * or on the launch geometry — shards and batch sizes agree bit for bit.
 * One launch on the handle's stream (one workgroup per env), no allocation, no synchronisation; capturable under srlhip_graph_begin.
 * SRLHIP_EINVAL: a null policy, a wrong struct_size, reserved != 0, null params / images / act_out, freeze_after_done without the
 * frozen plane, a pending srlhip_step_async.  SRLHIP_ENOTSUP: a host-pointer handle; an obs_mode other than raw pixels; a side outside
 * 43..224 (the message names the bound); sample on a continuous action mode (the message names "discrete").  A resident persistent
 * kernel parks. */
typedef struct srlhip_cnn_policy {
    int32_t struct_size;        /* sizeof(srlhip_cnn_policy): ABI check */
    int32_t per_env;            /* 1: params [num_envs][P]; 0: one [P] for every env */
    int32_t freeze_after_done;  /* as in srlhip_linear_policy */
    int32_t reserved;           /* 0 */
    const float *params;        /* a device pointer */
} srlhip_cnn_policy;
int srlhip_cnn_policy_act(srlhip_handle h, const srlhip_cnn_policy *pol, int32_t sample, const uint8_t *images,
                          const uint8_t *done_prev, uint8_t *frozen, void *act_out, float *score_out);
/* P of srlhip_cnn_policy for a frame of C channels, H x W, and A outputs; 0 for a shape the call refuses (no handle, no GPU needed) */
int64_t srlhip_cnn_param_count(int32_t channels, int32_t img_h, int32_t img_w, int32_t outputs);

/* The LINEAR policy's action from the frame: srlhip_cnn_policy_act for ARS with --srl-model raw_pixels
 * (rl_baselines/evolution_strategies/ars.py:85,162-166: np.dot(obs.reshape(-1), M +- noise * delta_k) on the uint8 frame as it lies — no
 * / 255, no VecNormalize).  The call follows srlhip_cnn_policy_act: device-pointer handles only (SRLHIP_ENOTSUP otherwise), cfg.obs_mode =
 * raw pixels (SRLHIP_ENOTSUP otherwise), any env kind and model, any frame a handle can have (sides 8..1024, C = 3, or 6 with multi_view).
 *   images     uint8 [num_envs][H][W][C], the plane srlhip_step / srlhip_reset write; a frame is the vector x of D = H W C bytes, NHWC.
 *   weights    float64 M [D][A], A = num_actions or action_dim of the handle; delta float64 [num_envs / 2][D][A] (paired) or NULL.
 *   paired = 1 env 2k acts with M + noise delta[k], env 2k + 1 with M - noise delta[k], k counted inside this handle (num_envs even): the
 *              ARS directions as the population lies in the batch; delta[k] is read once for both.  paired = 0: every env acts with M.
 *   done_prev, frozen, act_out: as in srlhip_policy_act (the `None` rows of frozen envs included).
 *   score_out  NULL, or float64 [num_envs][A]: the scores as they stood in front of the selection (frozen envs included).
 *   selection  discrete: the strict argmax, lowest index first; continuous: the row (float)score_a.  No sampling: a learner that samples
 *              draws from score_out.
 * ARITHMETIC (csrc/pixel_policy.hpp is its one text for device and host, -ffp-contract=off on both sides: the device's scores equal the
 * host program's bit for bit), all float64, no product fused with a sum: t = noise * delta[k][d][a]; w = M[d][a] + t (env 2k) or
 * M[d][a] - t (env 2k + 1), w = M[d][a] unpaired; term_d = (double)x_d * w; score_a = the sum of the D terms in THIS ORDER, a function of
 * (D, A) alone: the rows d are cut into chunks of 2048 (the last one ragged); inside chunk c, 256 virtual lanes: lane v owns the rows
 * 2048 c + v + 256 j, j = 0, 1, ..., and adds their terms in that order to a partial that starts from +0.0 (rows >= D add nothing); the
 * 256 partials meet in a pairwise tree, far halves first: p[i] = p[i] + p[i + h] for every i < h, for h = 128, 64, ..., 1; p[0] is the
 * chunk's sum; score_a = chunk 0's sum, + chunk 1's, + chunk 2's, ... in ascending order.  Against any other float64 summation of the
 * same terms |score_a - s| <= (8 + 8 + chunks) 2^-53 sum_d x_d |w_d[a]| to first order (tests/pixel_policy_ref.py).
 * The result for env e depends on its frame, M, its direction's delta block, noise, done_prev[e] and frozen[e] alone: not on num_envs, on
 * e, or on the launch geometry (a small population's launch gives every chunk a workgroup of its own and adds the chunk sums in the same
 * order) — shards and batch sizes agree bit for bit.
 * One kernel launch on the handle's stream, no allocation, no synchronisation; capturable under srlhip_graph_begin.  A resident persistent kernel parks.
 * SRLHIP_EINVAL: a null policy, a wrong struct_size, reserved != 0, null weights / images / act_out, paired without delta, delta without
 * paired, paired with an odd num_envs, freeze_after_done without the frozen plane, a pending srlhip_step_async.  SRLHIP_ENOTSUP: a
 * host-pointer handle; an obs_mode other than raw pixels. */
typedef struct srlhip_pixel_policy {
    int32_t struct_size;        /* sizeof(srlhip_pixel_policy): ABI check */
    int32_t paired;             /* 1: the ARS directions (above); 0: delta must be NULL */
    int32_t freeze_after_done;  /* as in srlhip_linear_policy */
    int32_t reserved;           /* 0 */
    const double *weights;      /* M [D][A], a device pointer */
    const double *delta;        /* [num_envs / 2][D][A], a device pointer, or NULL */
    double noise;               /* nu */
} srlhip_pixel_policy;
int srlhip_pixel_policy_act(srlhip_handle h, const srlhip_pixel_policy *pol, const uint8_t *images,
                            const uint8_t *done_prev, uint8_t *frozen, void *act_out, double *score_out);

/* The sampled selection on a SCORE PLANE the caller holds on the device: what puts sampling behind srlhip_pixel_policy_act(score_out) and
 * srlhip_policy_act(linear, score_out).  Device-pointer handles only, discrete action modes only, ANY env kind, model and observation
 * mode: the call reads the handle's action space (A = num_actions) and its action-stream counters, never the env state.
 *   scores     float64 [num_envs][A]
 *   frozen     uint8 [num_envs] or NULL: an env whose byte is non-zero gets -1 (the plane a policy call with freeze_after_done keeps)
 *   act_out    int32 [num_envs]
 * The draw of srlhip_rollout_mlp_policy_sampled word for word on the given scores (m, w_k, c_k, z, a; exp from the device math library;
 * the one text of csrc/policy_act.hpp), with u from the Philox block at the env's CURRENT action-stream counter c, stream 1.
 * COUNTER: the call leaves c + 1 for EVERY env, frozen or not, and advances it inside the kernel — a captured call draws fresh numbers
 * at every replay; K calls from c0 use the blocks c0 .. c0 + K - 1 that a fused sampled rollout with T = K uses.
 * The result for env e depends on its own score row, frozen[e] and its counter alone: not on num_envs, on e, or on the launch
 * geometry — shards and batch sizes agree bit for bit.
 * One launch on the handle's stream, no allocation, no synchronisation; capturable under srlhip_graph_begin.  A resident persistent
 * kernel parks.  SRLHIP_EINVAL: null scores or act_out, a pending srlhip_step_async.  SRLHIP_ENOTSUP: a host-pointer handle; a
 * continuous action mode (the message names "discrete"). */
int srlhip_sample_actions(srlhip_handle h, const double *scores, const uint8_t *frozen, int32_t *act_out);

/* Raw state access (checkpoint / parity): field ids below; arrays are
 * [num_envs] (or [k][num_envs] for vector fields) of the field's own type.
 * Always HOST pointers. */
#define SRLHIP_F_POS_X          0   /* f64 */
#define SRLHIP_F_POS_Y          1   /* f64 */
#define SRLHIP_F_TARGET_X       2   /* f64 (current target for 2Target)      */
#define SRLHIP_F_TARGET_Y       3   /* f64 */
#define SRLHIP_F_STEP_COUNT     4   /* i32 _env_step_counter                 */
#define SRLHIP_F_CUR_TARGET     5   /* i32 current_target (2Target)          */
#define SRLHIP_F_LAST_REWARD    6   /* f64 reward of the last step, uncast   */
#define SRLHIP_F_EP_RETURN      7   /* f64 running episode return            */
#define SRLHIP_F_EP_LENGTH      8   /* i32 running episode length            */
#define SRLHIP_F_LAST_RETURN    11  /* f64 return of the last finished episode (Monitor's r) */
#define SRLHIP_F_LAST_LENGTH    12  /* i32 its length (Monitor's l)          */
#define SRLHIP_F_N_FINISHED     13  /* i32 episodes finished so far          */
#define SRLHIP_F_TARGET2_X      9   /* f64 second target (2Target)           */
#define SRLHIP_F_TARGET2_Y      10  /* f64 */
#define SRLHIP_F_KUKA_Q         16  /* f64[7]  arm joint positions           */
#define SRLHIP_F_KUKA_QD        17  /* f64[7]  arm joint velocities          */
#define SRLHIP_F_KUKA_EE_TARGET 18  /* f64[3]  Kuka.end_effector_pos         */
#define SRLHIP_F_KUKA_BUTTON_Q  19  /* f64[2]  glider position, velocity     */
#define SRLHIP_F_KUKA_BUTTON_POS 20 /* f64[3]  button_pos (target)           */
#define SRLHIP_F_KUKA_GRIPPER   21  /* f64[3]  getArmPos()                   */
#define SRLHIP_F_KUKA_COUNTERS  22  /* i32[3]  n_contacts, n_steps_outside, terminated */
#define SRLHIP_F_KUKA_BUTTON_XY 23  /* f64[2]  button base position on the table */
#define SRLHIP_F_KUKA_BUTTON2_Q 24  /* f64[2]  Kuka2Button: second glider position, velocity */
#define SRLHIP_F_KUKA_BUTTON2_XY 25 /* f64[2]  Kuka2Button: second button base position */
#define SRLHIP_F_KUKA_GOAL      26  /* i32[2]  Kuka2Button: goal_id, n_contacts[1] (n_contacts[0] is COUNTERS[0]) */
#define SRLHIP_F_KUKA_OBJECTS   27  /* f64[30] KukaRandButton: (x, y, present) of the ten distractor objects */
#define SRLHIP_F_KUKA_GRIPPER_Q 28  /* f64[5]  full model: joints 7, 8, 10, 11, 13 (gripper_to_arm, left finger, left tip, right finger, right tip) */
#define SRLHIP_F_KUKA_GRIPPER_QD 29 /* f64[5]  their velocities */
#define SRLHIP_F_KUKA_BODIES     30 /* f64[66] KukaRandButtonGymEnv, full model: (x y z vx vy vz) of the ten distractors (draw order) and the ball */
/* IK conditioning flag of the full model (no counterpart in the reference; it qualifies the parity claim of this library).
 * Kuka.applyAction's damped-least-squares IK (kuka.py:41-42 jd = 1e-5, kuka.py:144-156) has a gain of up to 1 / (2 sqrt(jd)) = 158
 * along a vanishing singular direction of the arm's Jacobian: while the arm is driven through the neighbourhood of a kinematic
 * singularity (e.g. the elbow joint through 0 with a saturating policy at the far edge of the workspace box), the closed loop
 * IK -> position motors -> IK amplifies float64 rounding differences by ~2.4x per step, so NO two float64 implementations (PyBullet
 * included) agree to 1e-4 on joint positions, or bit for bit on reward / done, after such a crossing.  Bit 0 of the value: sticky
 * per episode, set when an IK solve of the episode had det(J^T J + jd I) < SRLHIP_KUKA_IK_CROSS_DET (random-agent rollouts stay
 * above 1e-7, amplification starts near 1e-9), cleared by the episode's reset.  value >> 1: env-steps taken with the bit set since the
 * handle was created.  Parity with the oracle (tests/) is asserted on every env-step BEFORE the bit. */
#define SRLHIP_F_KUKA_IK_CROSSED 31 /* i32     full model: (flagged env-steps << 1) | sticky bit */
#define SRLHIP_KUKA_IK_CROSS_DET 3e-9
int srlhip_get_state(srlhip_handle h, int32_t field, void *out);
int srlhip_set_state(srlhip_handle h, int32_t field, const void *in);
/* Zero-copy hand-off of a field's device array (e.g. to torch via
 * __cuda_array_interface__). */
int srlhip_device_ptr(srlhip_handle h, int32_t field, void **dptr);

/* Replaces <Env>.render("rgb_array") (kuka_button_gym_env.py:370-420, mobile_robot_env.py:282-334)
 * for the whole batch: uint8 [num_envs][img_h][img_w][3 (6 with multi_view / fpv)] of the CURRENT state,
 * produced by the tile rasteriser.  Also what step()/reset()/rollout() write to obs_out when
 * cfg.obs_mode == SRLHIP_OBS_RAW_PIXELS.  img_out follows cfg.io_device. */
int srlhip_render(srlhip_handle h, void *img_out);

/* ---- JPEG encoding of device-resident frames (dataset recording) ------------------------------------------------------------
 * Replaces the per-frame cv2.imwrite of the recorder (state_representation/episode_saver.py saveImage; here Pillow's
 * save(quality=95) in srlhip/recorder.py) and the copy of every raw frame to the host in front of it, for a whole batch.
 * images_dev uint8 [n][H][W][C] on device_id, H and W in 8..1024, C = 3 -> one stream per frame, C = 6 (multi_view / fpv) -> two:
 * stream 2i = channels 0..2 of frame i, stream 2i + 1 = channels 3..5 (the recorder's _1.jpg / _2.jpg).  n_streams = n * C / 3.
 * blob_dev needs n_streams * cap_per_stream bytes; stream s is blob_dev[offsets_dev[s] .. offsets_dev[s + 1]) — the streams are packed
 * back to back, bytes at and past offsets_dev[n_streams] are never written.  A stream larger than cap_per_stream is not written:
 * overflow_dev[s] = 1 (else 0) and its length in offsets_dev is 0.  The call only enqueues (three launches) on hip_stream (NULL = the
 * default stream), allocates nothing and may be captured into a graph.  SRLHIP_EINVAL: quality outside 1..100, C not 3 or 6, a side
 * outside 8..1024, a null buffer.
 *
 * FORMAT: baseline sequential JFIF that every libjpeg reads — SOI, APP0 (JFIF 1.01, no units, 1:1), DQT 0 and 1 (8-bit), SOF0 (Y 2x2,
 * Cb 1x1, Cr 1x1: 4:2:0), DHT DC0 AC0 DC1 AC1 (the Annex K.3 tables), DRI = 1 MCU, SOS, entropy-coded data, EOI:
 * srlhip_jpeg_header_bytes() = 629 bytes in front of the data.  Every 16x16 MCU is followed by RSTm (m = MCU index mod 8), the last one
 * by EOI, so every MCU starts byte-aligned from DC predictor 0.  The last byte of an MCU is padded with 1-bits; 0x00 follows every
 * 0xFF of the data.  MCU order: rows top to bottom, left to right; inside an MCU Y0 Y1 (top) Y2 Y3 (bottom), Cb, Cr.
 *
 * ARITHMETIC CONTRACT (integers only; csrc/jpeg.hpp is its one implementation for device and host, tests/jpeg_ref.py restates it in
 * numpy; >> is an arithmetic shift, / truncates):
 *   padding   pixel (y, x) past the frame reads pixel (min(y, H - 1), min(x, W - 1))
 *   colour    Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *             Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *             Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16          (all within 0..255, no clamp needed)
 *   chroma    the Cb (Cr) of a 2x2 cell is (a + b + c + d + 2) >> 2 of its four pixels' Cb (Cr), taken after the padding
 *   shift     every sample - 128
 *   DCT       K[u][x] = round(4096 s(u) cos((2x + 1) u pi / 16)), s(0) = 1 / sqrt 2, s(u > 0) = 1: K[0][x] = 2896, the other rows hold
 *             +- 4017 3784 3406 2896 2276 1567 799.  Rows first: r[y][u] = (sum_x K[u][x] p[y][x] + 2^8) >> 9 (16 x the orthonormal
 *             1-D transform, |r| <= 8034); then columns: c[v][u] = (sum_y K[v][y] r[y][u] + 2^13) >> 14 — c is 8 x the orthonormal
 *             2-D DCT, the scale libjpeg's integer DCT hands its quantiser.  All sums are exact in int32 (< 2^28).
 *   quantiser t = clamp((base * scale + 50) / 100, 1, 255), base = the Annex K.1 (Y) / K.2 (Cb, Cr) entry, scale = 5000 / quality for
 *             quality < 50, else 200 - 2 quality (libjpeg's rule); with d = 8 t:  q = sign(c) * ((|c| + d / 2) / d)  (half away from zero)
 *   coding    zigzag order; DC: difference to the previous block of the component INSIDE the MCU (Y0 -> Y1 -> Y2 -> Y3 from 0; Cb and Cr
 *             from 0), category code + category bits; AC: (run, category) codes, ZRL for every 16 zeros in front of a non-zero
 *             coefficient, EOB when the block ends in zeros; negative values v as the low bits of v - 1. */
int srlhip_jpeg_encode(int32_t device_id, const uint8_t *images_dev, int32_t n, int32_t img_h, int32_t img_w, int32_t n_channels,
                       int32_t quality, uint8_t *blob_dev, int64_t cap_per_stream, int64_t *offsets_dev, int32_t *overflow_dev,
                       void *hip_stream);
/* srlhip_render + srlhip_jpeg_encode on the handle's stream: rasterises the CURRENT state of every env into the handle's scratch exactly
 * as srlhip_render does and encodes those frames (num_envs streams, 2 num_envs with multi_view / fpv).  Pointers follow cfg.io_device;
 * cap_per_stream = blob_cap / n_streams.  A host-pointer handle copies offsets_out [n_streams + 1] and overflow_out [n_streams] first,
 * then only the offsets_out[n_streams] bytes of blob that were written.  SRLHIP_EINVAL while a srlhip_step_async is pending; a
 * resident kernel parks. */
int srlhip_render_jpeg(srlhip_handle h, int32_t quality, void *blob_out, int64_t blob_cap, int64_t *offsets_out, int32_t *overflow_out);
/* Host only: the size of the header in front of the entropy-coded data (the smallest stream is this + one MCU + EOI). */
size_t srlhip_jpeg_header_bytes(void);
/* Host only, no GPU needed: ONE stream through the same source on the CPU (pixel (y, x) at image + (y * img_w + x) * pix_stride, three
 * bytes R G B; pix_stride >= 3) — so that the arithmetic above can be checked without a device.  *len = the stream's size; when it
 * exceeds cap nothing is written and the call returns SRLHIP_ENOMEM. */
int srlhip_jpeg_encode_host(const uint8_t *image, int32_t img_h, int32_t img_w, int32_t pix_stride, int32_t quality, uint8_t *out,
                            size_t cap, size_t *len);

/* ---- JPEG decoding of the library's own streams where they lie on the device (reading a recorded dataset) --------------------
 * The inverse of srlhip_jpeg_encode, for exactly the streams it writes; every other JPEG is refused, never mis-decoded (Pillow stays
 * the reader for those).  blob_dev / offsets_dev [n_streams + 1] have srlhip_jpeg_encode's layout: stream s is
 * blob_dev[offsets_dev[s] .. offsets_dev[s + 1]).  images_dev uint8 [n_streams * 3 / C][H][W][C]: C = 3 -> one frame per stream, C = 6 ->
 * streams 2i and 2i + 1 become channels 0..2 and 3..5 of frame i (n_streams even).  workspace_dev: 16-byte aligned,
 * srlhip_jpeg_decode_workspace_bytes(n_streams, H, W) bytes (0 = these sizes are refused), contents undefined afterwards.  The call only
 * enqueues (five launches) on hip_stream (NULL = the default stream), allocates nothing and may be captured into a graph.
 * SRLHIP_EINVAL: C not 3 or 6, a side outside 8..1024, n_streams negative, odd with C = 6 or with more than 2^31 / 6 MCUs in all, a
 * null buffer, a misaligned workspace.
 *
 * status_dev[s]: 0 decoded; 1 the first 629 bytes are not the accepted layout for this H, W; 2 empty stream (the length 0 an overflowed
 * encode leaves); 3 entropy-coded data malformed.  A frame (C = 6: a view) whose status is not 0 is written as zeros.
 *
 * ACCEPTED LAYOUT: the 629 bytes srlhip_jpeg_encode writes in front of the data for sides H, W — SOI, APP0 (JFIF 1.01), two 8-bit DQT
 * (ids 0, 1), SOF0 (8 bits, 3 components, Y 2x2 table 0, Cb and Cr 1x1 table 1), the four Annex K.3 DHT, DRI = 1, SOS — compared byte
 * for byte, EXCEPT the 2 x 64 table values (bytes 25..88 and 94..157), which are read and used, whatever they are.  Behind them the
 * data: a byte 0xFF whose successor is not 0x00 (or is missing) is a marker; there must be exactly n_mcus = ceil(H / 16) ceil(W / 16) of
 * them, the k-th being RST(k mod 8) and the last EOI as the stream's final two bytes — else status 3.  MCU k is the bytes between
 * marker k - 1 (the header for k = 0) and marker k.  Streams of 2^30 bytes or more: status 3.
 *
 * SAFETY: every read of blob_dev lies inside the stream's own [offsets_dev[s], offsets_dev[s + 1]) and, while an MCU is decoded, inside
 * that MCU's bytes; every write inside images_dev's n_streams / (C / 3) frames, status_dev's n_streams words and the workspace.  An MCU
 * reads at most 6 x 64 symbols whatever its bytes hold.
 *
 * ARITHMETIC CONTRACT (integers only; csrc/jpeg_decode.hpp is its one implementation for device and host, tests/jpeg_decode_ref.py
 * restates it in numpy; >> is an arithmetic shift).  It restates what libjpeg does by default, so that Pillow and this decoder give
 * the same frame:
 *   bits      most significant first; the 0x00 behind an 0xFF is dropped.  Blocks per MCU: Y0 Y1 (top) Y2 Y3 (bottom), Cb, Cr; Y uses
 *             DC / AC table 0 and DQT 0, Cb and Cr table 1 and DQT 1.  Bits past the MCU's last byte: status 3 once one is consumed.
 *   DC        category n (0..11), then n bits v: diff = v when v >= 2^(n - 1), else v - 2^n + 1 (the encoder's rule inverted);
 *             DC = previous block's DC of the component INSIDE the MCU (Y0 -> Y1 -> Y2 -> Y3 from 0; Cb, Cr from 0) + diff
 *   AC        k = 1; symbol (run, size): size 0, run 15 -> k += 16, and k > 63 is status 3 (a coefficient must follow a ZRL); size 0,
 *             other run -> the block ends (EOB); else k += run, k > 63 is status 3, coefficient k of the zigzag scan = size bits
 *             extended as above, k += 1; the block also ends at k = 64.  Sixteen bits that are no code: status 3.
 *   dequant   coefficient * the DQT's k-th value, kept in 16 bits (two's complement wrap; exact for every stream the encoder writes)
 *   IDCT      libjpeg's slow-integer inverse DCT.  One 8-point pass on x0..x7, constants round(c 2^13):
 *               z = (x2 + x6) 4433;  t2 = z - x6 15137;  t3 = z + x2 6270;  t0 = (x0 + x4) << 13;  t1 = (x0 - x4) << 13
 *               t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2
 *               z5 = (x7 + x3 + x5 + x1) 9633;  z1 = -(x7 + x1) 7373;  z2 = -(x5 + x3) 20995
 *               z3 = z5 - (x7 + x3) 16069;  z4 = z5 - (x5 + x1) 3196
 *               o0 = x7 2446 + z1 + z3;  o1 = x5 16819 + z2 + z4;  o2 = x3 25172 + z2 + z3;  o3 = x1 12299 + z1 + z4
 *               y0, y7 = t10 +- o3;  y1, y6 = t11 +- o2;  y2, y5 = t12 +- o1;  y3, y4 = t13 +- o0;  each (y + 2^(S - 1)) >> S
 *             first down every column with S = 11 (two extra bits kept), then along every row with S = 18.  Sums are 32-bit two's
 *             complement (they wrap; on the encoder's streams none does).  sample = libjpeg's range-limit table on the low 10 bits t
 *             of the result: t + 128 for t < 128, 255 for t < 512, 0 for t < 896, else t - 896 — that is clamp(value + 128, 0, 255)
 *             for every value in -512..511.
 *   upsample  libjpeg's "fancy" 2x2 upsampling of the ceil(H / 2) x ceil(W / 2) REAL chroma samples (what lies past them in the padded
 *             MCUs is not used; rows and columns past the edge repeat the edge).  For pixel (y, x): r = y >> 1, c = x >> 1, the farther
 *             row f = r - 1 for even y, r + 1 for odd y (clamped); column sums s[j] = 3 p[r][j] + p[f][j];
 *             even x: (3 s[c] + s[c - 1] + 8) >> 4, at c = 0 (4 s[c] + 8) >> 4;  odd x: (3 s[c] + s[c + 1] + 7) >> 4, at the last
 *             column (4 s[c] + 7) >> 4
 *   colour    with cb = Cb - 128, cr = Cr - 128:  R = clamp(Y + ((91881 cr + 32768) >> 16)),
 *             G = clamp(Y + ((-22554 cb - 46802 cr + 32768) >> 16)),  B = clamp(Y + ((116130 cb + 32768) >> 16)), clamp to 0..255
 *   crop      pixel (y, x) for y < H, x < W
 * AGAINST PILLOW (12.2, libjpeg-turbo; tests/test_jpeg_decode_cpu.py, on the CPU): over 74 streams of the encoder (8x8 .. 224x224, six
 * kinds of frame, quality 10 / 50 / 95 / 100; 441 600 samples) the maximum |difference| to Image.open(...).convert("RGB") is 0 and 0
 * samples differ: equality is reached. */
int srlhip_jpeg_decode(int32_t device_id, const uint8_t *blob_dev, const int64_t *offsets_dev, int32_t n_streams, int32_t img_h,
                       int32_t img_w, int32_t n_channels, uint8_t *images_dev, int32_t *status_dev, void *workspace_dev, void *hip_stream);
/* Host only: the bytes of workspace srlhip_jpeg_decode needs; 0 for sizes it refuses. */
size_t srlhip_jpeg_decode_workspace_bytes(int32_t n_streams, int32_t img_h, int32_t img_w);
/* Host only, no GPU needed: 0 and the sides when stream[0 .. len) starts with the accepted layout (only the 629 header bytes are
 * read; img_h / img_w may be NULL), else SRLHIP_ENOTSUP. */
int srlhip_jpeg_probe(const uint8_t *stream, size_t len, int32_t *img_h, int32_t *img_w);
/* Host only, no GPU needed: ONE stream through the same source on the CPU, the sides taken from its header; pixel (y, x) is written at
 * out + (y * W + x) * pix_stride, three bytes R G B (pix_stride >= 3: a view of a 6-channel frame is written in place); out_cap = the
 * bytes available at out, at least (H W - 1) pix_stride + 3, else SRLHIP_ENOMEM.  Returns 0 with *status = 0 (decoded) or 3 (zeros
 * written); SRLHIP_ENOTSUP with *status = 1 or 2 when the header is not accepted (nothing is written).  status may be NULL. */
int srlhip_jpeg_decode_host(const uint8_t *stream, size_t len, uint8_t *out, int32_t pix_stride, size_t out_cap, int32_t *status);

/* ---- JPEG decoding of baseline streams as libjpeg writes them by default (reading a dataset any recorder wrote) ---------------
 * What srlhip_jpeg_decode refuses: the files of Pillow's save() (srlhip/recorder.py) and of cv2.imwrite (the reference's
 * state_representation/episode_saver.py) — 4:2:0 or 4:4:4, the Annex K.3 Huffman tables, any restart interval or none.  Everything
 * not named differently here is srlhip_jpeg_decode's: the layout of blob_dev / offsets_dev / images_dev, the pairing of streams 2i,
 * 2i + 1 for C = 6, sides 8..1024, status 0 / 1 (header not accepted, or its sides are not the call's H, W) / 2 (empty stream) / 3
 * (entropy-coded data malformed; also streams of 2^30 bytes or more), zeros for a frame or view whose status is not 0, the
 * SRLHIP_EINVAL rules (the bound on the call's size is n_streams * blocks < 2^31 with blocks as below), the 16-byte aligned workspace
 * of srlhip_jpeg_decode_baseline_workspace_bytes(n_streams, H, W) bytes (0 = these sizes are refused).  The call only enqueues (five
 * launches) on hip_stream, allocates nothing, does no host synchronisation and may be captured into a graph.  The workspace is sized
 * for the worse of the two sampling modes — blocks = max(6 ceil(H / 16) ceil(W / 16), 3 ceil(H / 8) ceil(W / 8)) per stream, 192 bytes
 * per block, 272 bytes of descriptor per stream — so that one call may mix them.
 * TUNING OVERRIDE: the entropy launch gives a stream to the first L lanes of every wavefront; L = 4 is built in (profiles/NOTES.md BB has
 * the measurement).  The environment variable SRLHIP_JPEG_BASELINE_LANES = 64, 16 or 4, read at every call, replaces L for that call
 * (any other value is ignored); the frames and status words do not depend on it.  profiles/jpeg_baseline_decode_microbench.py uses it.
 *
 * ACCEPTED LAYOUT: SOI, then marker segments (FF, marker, 16-bit length, body) up to SOS; at most 64 segments, more is status 1.
 *   APP0..APP13, APP15, COM   skipped by their length.  APP14 (Adobe) is status 1: it can change the colour transform.
 *   DQT    8-bit precision only, ids 0..3, several tables per segment allowed, a later definition replaces an earlier one.
 *   SOF0   only, once: 8 bits, 3 components with ids 1, 2, 3 in that order, sampling (2x2, 1x1, 1x1) or (1x1, 1x1, 1x1), Tq 0..3;
 *          every Tq refers to a table defined before SOS.
 *   DHT    class 0 / 1, id 0 / 1, several tables per segment allowed; every table must be, byte for byte, the Annex K.3 luminance or
 *          chrominance table of its class (either may stand under either id).  Optimised tables are status 1.
 *   DRI    any interval Ri, 0 = none.
 *   SOS    3 components in frame order, every table selector 0 / 1 and defined, Ss = 0, Se = 63, Ah = Al = 0.
 *   Any other marker in front of SOS is status 1: SOF1 / 2 / .., DAC, DNL, a second SOF, RST, EOI, a fill byte.
 * Behind SOS lies one interleaved scan of ceil(H / 16) ceil(W / 16) MCUs of 6 blocks (4:2:0: Y0 Y1 Y2 Y3 Cb Cr) or ceil(H / 8) ceil(W / 8)
 * MCUs of 3 blocks (4:4:4: Y Cb Cr), rows top to bottom, left to right.
 *   bits      most significant first; the 0x00 behind an 0xFF is dropped.  An 0xFF followed by anything but 0x00, or by nothing, ends
 *             the data there: bits past it, or past the stream's end, are status 3 once one is consumed.  Bytes behind the last MCU
 *             are not read.
 *   DC        prediction runs per component ACROSS MCUs, from 0 at the start of the scan and after each restart
 *   restart   with Ri > 0, after every Ri MCUs except behind the last one: the remaining bits of the current byte are dropped and the
 *             next two bytes must be FF D0+(k mod 8) for the k-th restart (k from 0); anything else is status 3
 *   symbols   category, extension, ZRL, EOB and k > 63 rules are srlhip_jpeg_decode's (DC, AC above); a component uses the K.3 tables
 *             its SOS selectors name and the DQT its Tq names.  A stream is decoded with at most blocks x 64 symbols.
 * Dequantisation (16-bit wrap), IDCT, range limit, fancy upsampling over the real ceil(H / 2) x ceil(W / 2) chroma samples, colour and
 * crop are srlhip_jpeg_decode's ARITHMETIC CONTRACT.  For 4:4:4 there is no upsampling: Cb and Cr are taken at the pixel.
 * csrc/jpeg_baseline.hpp is the one implementation for device and host, tests/jpeg_baseline_ref.py restates it in numpy.
 * The library's own streams are baseline streams with Ri = 1 and decode through this call to the same frames.
 *
 * SAFETY: every read of blob_dev lies inside the stream's own [offsets_dev[s], offsets_dev[s + 1]) (the data is fetched in aligned
 * 16-byte pieces; a piece that reaches across the stream's first or last byte is read byte by byte instead); every write inside
 * images_dev's n_streams / (C / 3) frames, status_dev's n_streams words and the workspace.
 *
 * AGAINST PILLOW (12.2, libjpeg-turbo; tests/test_jpeg_baseline_cpu.py, on the CPU): over the streams of
 * tests/golden/jpeg_baseline_pillow.npz, written by Pillow (sizes 8x8 .. 224x224 with odd ones, six kinds of frame, quality 10 / 50 /
 * 95 / 100, 4:2:0 and 4:4:4, with and without restart markers), 0 samples differ from Image.open(...).convert("RGB"). */
int srlhip_jpeg_decode_baseline(int32_t device_id, const uint8_t *blob_dev, const int64_t *offsets_dev, int32_t n_streams, int32_t img_h,
                                int32_t img_w, int32_t n_channels, uint8_t *images_dev, int32_t *status_dev, void *workspace_dev,
                                void *hip_stream);
/* Host only: the bytes of workspace srlhip_jpeg_decode_baseline needs; 0 for sizes it refuses. */
size_t srlhip_jpeg_decode_baseline_workspace_bytes(int32_t n_streams, int32_t img_h, int32_t img_w);
/* Host only, no GPU needed: 0, the sides and the sampling (420 or 444) when the segments of stream[0 .. len) up to SOS are the accepted
 * layout (nothing behind SOS is read; any of the three may be NULL), else SRLHIP_ENOTSUP. */
int srlhip_jpeg_probe_baseline(const uint8_t *stream, size_t len, int32_t *img_h, int32_t *img_w, int32_t *sampling);
/* Host only, no GPU needed: ONE stream through the same source on the CPU; arguments, return values and *status as
 * srlhip_jpeg_decode_host. */
int srlhip_jpeg_decode_baseline_host(const uint8_t *stream, size_t len, uint8_t *out, int32_t pix_stride, size_t out_cap, int32_t *status);

/* Per-env statistics of the most recently FINISHED episode and the number of
 * finished episodes: what stable_baselines.bench.Monitor records
 * (environments/utils.py:54).  HOST pointers, any may be NULL. */
int srlhip_episode_stats(srlhip_handle h, double *last_return, int32_t *last_length,
                         int32_t *n_finished);
/* The same two record planes WITHOUT a copy, for the per-step loop of rl_baselines.train (SubprocVecEnv's workers hand back
 * info['episode'] with the step's result, rl_baselines/utils.py:213-229; environments/utils.py:54): host-pointer handles
 * (cfg.io_device = 0) keep last_return [n] f64 / last_length [n] i32 in mapped pinned host memory that the step kernels write
 * directly.  The pointers stay valid until srlhip_destroy; entry i is final for the episode env i finished in a step once that
 * srlhip_step / srlhip_rollout call has returned.  EINVAL on device-pointer handles (use srlhip_episode_stats_device there). */
int srlhip_episode_records(srlhip_handle h, const double **last_return, const int32_t **last_length);

/* Same statistics for DEVICE-resident consumers (cfg.io_device-independent): enqueue-only on the handle's stream, no
 * host synchronisation.  last_return is narrowed to float32 — the element the multi-GPU path all-gathers over RCCL
 * (one all-gather of per-env episode returns per rollout).  DEVICE pointers, any may be NULL. */
int srlhip_episode_stats_device(srlhip_handle h, float *d_last_return, int32_t *d_last_length, int32_t *d_n_finished);

/* Stream ordering and live kernel timing (HIP events on the handle's stream). */
int srlhip_sync(srlhip_handle h);
/* Enqueue a copy of `bytes` bytes on the handle's stream, ordered with the steps / renders / encoder forwards enqueued there
 * (device <-> device, or device <-> PINNED host memory; the direction is taken from the pointers).  What a device-pointer caller
 * uses to feed actions and fetch reward / done / state planes without a second stream: the sharded HipVecEnv with a learned SRL
 * model moves only [n][state_dim] floats per step this way (the reference pickles a 150 KB frame per env and step through
 * MultiprocessSRLModel's queues, rl_baselines/utils.py:162-191).  Returns without waiting. */
int srlhip_copy_async(srlhip_handle h, void *dst, const void *src, size_t bytes);
int srlhip_stream(srlhip_handle h, void **hip_stream);
int srlhip_timing_begin(srlhip_handle h);
int srlhip_timing_end(srlhip_handle h, float *elapsed_ms);   /* synchronises */

/* HIP graphs for launch-bound step loops (cfg.io_device = 1 only): everything enqueued on the handle's stream between
 * graph_begin and graph_end — srlhip_step / srlhip_rollout / srlhip_render with device pointers, srlhip_encoder_forward
 * on srlhip_stream() — is captured instead of executed; srlhip_graph_launch() replays it (same buffers) with one launch.
 * Make one eager call of the same sequence first: lazily allocated scratch must exist before the capture. */
typedef struct srlhip_graph *srlhip_graph_handle;
int srlhip_graph_begin(srlhip_handle h);
int srlhip_graph_end(srlhip_handle h, srlhip_graph_handle *out);
int srlhip_graph_launch(srlhip_handle h, srlhip_graph_handle g);
int srlhip_graph_destroy(srlhip_graph_handle g);

/* The part of the Kuka-button model that is NOT pinned by the reference's own source: link frames, inertial parameters,
 * joint limits / damping of pybullet_data/kuka_iiwa/kuka_with_gripper2.sdf (loaded at kuka.py:60), the IK / gripper
 * reference points, the gripper's collision spheres, the table and button-base heights of table/table.urdf — recalled
 * from upstream in this repo, so kept as DATA: 138 doubles.  srlhip_kuka_default_model() returns the baked
 * table; srlhip_set_kuka_model() installs another one on a Kuka handle (before the next srlhip_reset): the settled state is
 * re-integrated, every following reset / step uses it.  A 7-joint serial arm whose joints turn about their local z is
 * assumed (joint_rpy = URDF rpy of the joint frame in the parent link frame, joint_xyz its origin; inertia = principal
 * moments about com, axes parallel to the link frame).  With a table installed the batch is stepped by the lane-group
 * kernel at any size; lumped Kuka2ButtonGymEnv handles return SRLHIP_ENOTSUP (full-model ones take srlhip_set_kuka_tree_model).  tests/golden/make_kuka_pybullet_golden.py
 * fills this struct from pybullet_data when PyBullet is importable. */
typedef struct srlhip_kuka_model {
    double joint_xyz[7][3], joint_rpy[7][3], joint_lower[7], joint_upper[7], joint_damping;
    double mass[7], com[7][3], inertia[7][3];
    double ee_point[3];          /* IK end effector (link_7 inertial frame) in the link_7 frame          */
    double gripper_point[3];     /* COM of gripper link 8 (getArmPos) in the link_7 frame                 */
    double sphere[6][4];         /* gripper collision spheres: centre in the link_7 frame, radius         */
    double table_top_z, button_base_z;
} srlhip_kuka_model;
int srlhip_kuka_default_model(srlhip_kuka_model *m);
int srlhip_set_kuka_model(srlhip_handle h, const srlhip_kuka_model *m);

/* The full model as data (SRLHIP_KUKA_MODEL_FULL): a kinematic tree of up to 12 revolute DoFs, parents before children.
 * Integer-valued fields are stored as doubles so that the struct is a flat table of 510 doubles.  Per DoF: parent (-1 = the fixed
 * base at kuka.py:63's pose), joint frame in the parent link (origin, fixed rotation Rj row-major: child = Rj * Rot(axis, q)),
 * unit axis in the joint frame, limits (lower > upper = none), damping, link mass / centre of mass / inertia about it in link axes
 * (xx xy xz yy yz zz; fixed-joint children are merged in exactly), the joint's POSITION_CONTROL motor (positionGain, force,
 * maxVelocity; velocityGain is 1), the pybullet joint index.  Then the IK end-effector link / point (kuka_end_effector_index 6),
 * the getArmPos() link / point (kuka_gripper_index 8: its COM), up to 16 collision spheres (link, centre, radius, combined lateral
 * friction), table / button-base heights, the per-step budget of limit + contact-normal rows (<= 6: the lane group's second row bank; values above are rejected) and the
 * friction switch, then the SOLVER DETAILS below.
 * Impulse bounds: a contact-normal row is boxed to [0, 1e10] (Bullet's default upper bound) in the oracle and in the kernel's general
 * path; the one-button contact fast path solves normal rows in u = lambda / 2^33 so that the projection is the hardware clamp of one add,
 * i.e. its upper bound is 2^33 = 8.59e9 — impulses are ~1e-2, neither bound is ever reached, the results are identical.
 * The arm part is in-tree or pinned elsewhere (srlhip_kuka_model); the gripper part is RECALLED from kuka_with_gripper2.sdf
 * [UNVERIFIED-MEMORY] — tests/golden/make_kuka_pybullet_golden.py overwrites it from pybullet_data when PyBullet is importable. */
typedef struct srlhip_kuka_tree_joint {
    double parent, xyz[3], Rj[9], axis[3], lower, upper, damping, mass, com[3], inertia[6], kp, max_force, max_vel, joint_index;
} srlhip_kuka_tree_joint;
typedef struct srlhip_kuka_tree_sphere { double link, c[3], r, mu; } srlhip_kuka_tree_sphere;
typedef struct srlhip_kuka_tree_model {
    double nd;
    srlhip_kuka_tree_joint j[12];
    double ee_link, ee_point[3], grip_link, grip_point[3], nsphere;
    srlhip_kuka_tree_sphere s[16];
    double table_top_z, button_base_z, max_generic_rows, friction;
    /* Details of the dependency's constraint solver (Bullet 2.87 btMultiBodyConstraintSolver as driven by pybullet 1.8.6:
     * kuka_button_gym_env.py:219-220 sets 150 iterations, :351 steps it) that this repo RECALLS and cannot read — kept as data so
     * that the day a PyBullet fixture exists, matching it is a choice of table values (tests/golden/fit_kuka_pin.py searches them on
     * the oracle), not a kernel change.  Defaults (0, 0.2, 0.2, 0) = the behaviour of rounds 1-3.
     *   solver_detail   bit mask of SRLHIP_KUKA_DETAIL_*
     *   contact_erp     error reduction of penetrating contact rows (Bullet m_erp2; pybullet's server is recalled to use 0.08)
     *   limit_erp       the same for joint-limit rows, the button's two stops included (Bullet m_erp)
     *   linear_slop     a contact row sees penetration = distance + linear_slop (Bullet m_linearSlop; recalled server value 1e-5) */
    double solver_detail, contact_erp, limit_erp, linear_slop;
} srlhip_kuka_tree_model;
#define SRLHIP_KUKA_DETAIL_ALT_SWEEP  1  /* the non-contact rows (motors, limits, button rows) are swept backwards on even iterations */
#define SRLHIP_KUKA_DETAIL_BODY_ORDER 2  /* non-contact rows in body-creation order: button (stops, motor) before the arm (limits, motors) */
#define SRLHIP_KUKA_DETAIL_FRICTION2  4  /* second friction row per contact along n x t1; the row budget becomes min(max_generic_rows, 4) */
int srlhip_kuka_tree_default_model(srlhip_kuka_tree_model *m);                   /* host only, no GPU needed */
/* Install a table on a SRLHIP_KUKA_MODEL_FULL handle: settled state and start-state table are re-integrated; reset afterwards. */
int srlhip_set_kuka_tree_model(srlhip_handle h, const srlhip_kuka_tree_model *m);

/* Which kernel steps this Kuka handle's batch: 2 = tree lane-group (full model, kuka_tree_rollout_k: every batch size), 1 = lane-group (16 lanes per env, kuka_group_rollout_k: batches up to 12288
 * envs), 0 = lane-per-env (kuka_rollout_k: larger batches and the lumped Kuka2ButtonGymEnv); the environment variable
 * SRLHIP_KUKA_KERNEL=group|lane overrides the choice.  Both read and write the same state and produce the same outputs
 * (to ~1e-11 on joint positions; discrete flags identical).  The tree kernel has a two-wavefronts-per-SIMD variant
 * (kuka_tree_rollout_occ_k: one-button envs, Cartesian actions) that the library uses from 65536 envs up;
 * SRLHIP_KUKA_OCC=0|1 forces either.  Same state, same outputs to the same bar. */
int srlhip_kuka_kernel(srlhip_handle h);

/* Diagnostic: runs every cross-lane primitive of the lane-group Kuka kernel (csrc/kuka_group.hpp: DPP row broadcasts and
 * shifts, row votes, the fused solver-row instructions, the lane-parallel Gauss-Jordan, the prefix-composed forward
 * kinematics for joint angles q7) on one wavefront of device_id and returns their per-lane results, out[40][64] doubles.
 * tests/test_gpu_group_primitives.py checks them against the definitions the CPU-side emulation of the same source uses. */
int srlhip_selftest_group_primitives(int32_t device_id, const double *q7, double *out, int32_t out_doubles);

/* Diagnostic, tests only: runs a small scripted draw program on every random generator form of the library (csrc/rng.hpp, csrc/kuka_group.hpp;
 * the interpreter is csrc/rng_probe.hpp) on device_id, without an env handle, and returns every drawn value as raw bits.
 *   generator  0 Mt19937 (one lane per env)   1 GroupMt (16 lanes per env)   2 Lane0Rng<Mt19937> (16 lanes, lane 0 draws)
 *              3 Philox (one lane per env, `stream` 0 / 1)   4 GroupPhilox (stream 0)   5 GroupActions (stream 1); 1, 2, 4, 5 write 16 lanes
 *   keys       uint32 [2][n_envs]: MT19937 seed digits (key_len [n_envs] = 1 or 2 of them, seeded by srlhip_seed's own kernel) / Philox key
 *   stride     MT forms: env stride of the state words in device memory (>= n_envs)
 *   mask       [n_envs] or NULL: an env with mask 0 never draws (its out rows stay 0, its state as seeded)
 *   state_in   NULL, or the start state in state_out's layout (MT: instead of seeding; Philox family: the start counters, default 0)
 *   script     int32 [n_ops][3] = (op, index of the first argument in args, repeat):  0 raw word (Philox: the 4 words of a block, forms 0 1 3)
 *              1 double01   2 uniform(lo, hi)   3 normal(loc, scale)   4 bounded(r) -> [0, r] (the only draw of form 5)
 *              5 store + load through the state in device memory, as at a kernel boundary   6 Philox family: counter = start counter + arg
 *   skip       int32 [n_envs]: draws env e throws away before its script: raw words (MT), blocks (form 3), normal(0, 1) (form 4), bounded(5) (form 5)
 *   out        uint64 [n_envs][lanes][values]: float64 bits / zero-extended integers, lanes = 16 for forms 1 2 4 5, else 1
 *   state_out  uint64 per env: MT forms 627 (624 state words, index, has_gauss, bits of the cached deviate), Philox family 1 (counter)
 * SRLHIP_EINVAL for a script the form cannot run or buffers too small for it. */
int srlhip_selftest_rng(int32_t device_id, int32_t generator, int32_t stream, int32_t n_envs, int32_t stride, const uint32_t *keys,
                        const int32_t *key_len, const uint8_t *mask, const uint64_t *state_in, const int32_t *script, int32_t n_ops,
                        const double *args, int32_t n_args, const int32_t *skip, uint64_t *out, int64_t out_words, uint64_t *state_out,
                        int64_t state_words);

const char *srlhip_last_error(srlhip_handle h);
int srlhip_abi_version(void);

/* ---- SRL encoder (raw_pixels -> state) ----------------------------------------------------------------
 * Replaces SRLNeuralNetwork.getState (state_representation/models.py:178-193: preprocessImage, the H/W
 * transpose, one CustomCNN forward) and the one-image-at-a-time encoder server MultiprocessSRLModel._run
 * (rl_baselines/utils.py:181-191) for a whole DEVICE-resident batch of frames.  Weights are plain float32 host
 * arrays in torch layout with the BatchNorms already folded into the preceding convolution
 * (w' = w*gamma/sigma, b' = beta - mu*gamma/sigma):
 *   conv1_w [64][C][7][7] conv1_b [64]   conv2_w, conv3_w [64][64][3][3]   conv2_b, conv3_b [64]
 *   fc_w [state_dim][64 * cells]  fc_b [state_dim]      (cells = the last pooled map's size, torch flatten order)
 * Covered shapes (srlhip_encoder_supported() tells beforehand, anything else -> SRLHIP_ENOTSUP and the caller keeps
 * the PyTorch-ROCm forward): frames of 8..1024 pixels a side that survive the three conv + pool stages, with C = 3
 * channels or C = 6 (multi_view / fpv: two cameras, kuka_button_gym_env.py:401-417).  64x64x3 (BASELINE configs 4-5)
 * runs as ONE fused kernel (csrc/encoder.hip); every other shape — the reference's 224x224 RENDER size among them —
 * runs layer by layer with f16 hi/lo activation planes in HBM (csrc/encoder_general.hip), same arithmetic.
 * images_dev uint8 [n][H][W][C] and states_dev float [n][state_dim] are DEVICE pointers on device_id; the call only
 * enqueues on hip_stream (NULL = the default stream).  The layered path keeps grow-only scratch planes per handle: a
 * caller that captures the forward into a HIP graph calls it once with its batch size before capturing. */
typedef struct srlhip_encoder *srlhip_encoder_handle;
int srlhip_encoder_supported(int32_t img_h, int32_t img_w, int32_t n_channels);
/* Host-only: inputs of the fully connected layer for this frame shape (64 channels x the last pooled map), 0 when the
 * shape is not covered — the second dimension fc_w must have. */
int32_t srlhip_encoder_feature_count(int32_t img_h, int32_t img_w, int32_t n_channels);
int srlhip_encoder_create(int32_t device_id, int32_t img_h, int32_t img_w, int32_t n_channels, int32_t state_dim,
                          const float *conv1_w, const float *conv1_b, const float *conv2_w, const float *conv2_b,
                          const float *conv3_w, const float *conv3_b, const float *fc_w, const float *fc_b,
                          srlhip_encoder_handle *out);
int srlhip_encoder_forward(srlhip_encoder_handle e, const uint8_t *images_dev, int32_t n, float *states_dev,
                           void *hip_stream);
/* Synchronises the device; *flag = 1 if an activation ever left float16's range (|x| >= 65504: the split-f16
 * matrix path then lost accuracy and the caller should use the PyTorch forward for these weights).
 * Watched: the pooled, rectified activations of layers 1 and 2 — the values that travel between layers as f16
 * hi / lo planes — in both kernels and every variant of them.  Layer 3's pooled features stay float32 and are not
 * watched: they may exceed 65504 without loss.  The flag is STICKY: a new handle starts with 0; once a forward has
 * set it, it stays 1 for the life of the handle — later forwards within range do not clear it, and neither does
 * reading it (it describes the weights, which a handle never changes).  Below the line the states keep the
 * accuracy of the float32 forward (tests/test_gpu_encoder_f64.py, tests/test_gpu_encoder_overflow.py: pooled
 * maxima of 65504 / 2 hold the same bar as ordinary weights; at 2 x 65504 the flag is set and the states are
 * not to be used). */
int srlhip_encoder_overflow(srlhip_encoder_handle e, int32_t *flag);
/* Diagnostic: one synchronous forward whose workgroup 0 stamps the shader clock (s_memtime) at nine points of its
 * first frames; cycles9[k] = cycles between stamp k and k+1, slowest wave, averaged over frames:
 * 0 unpack, 1 layer-1 MFMA + pooling, 2 barrier, 3 layer-2 k-loop, 4 layer-2 epilogue, 5 barrier, 6 layer 3,
 * 7 FC, 8 loop turn-around.  Used by bench.py / DESIGN.md to attribute the kernel's time. */
int srlhip_encoder_phase_cycles(srlhip_encoder_handle e, const uint8_t *images_dev, int32_t n, float *states_dev,
                                int64_t *cycles9);
int srlhip_encoder_destroy(srlhip_encoder_handle e);
const char *srlhip_encoder_last_error(srlhip_encoder_handle e);
/* Host-only, layered path: layer 1's B-operand image for 3- or 6-channel frames — [channel half][k-step][lane][8 hi | 8 lo]
 * f16 with k = (ky * 8 + kx) * cpix + c (cpix = 4 or 8 staged f16 per pixel: the channels, the validity mask, zero fill; kx = 7
 * is a zero slot), 2 * (7 * 8 * cpix / 16) * 2048 bytes; *scale = the power-of-two pre-scale. */
int srlhip_encoder_pack_first_layer(int32_t n_channels, const float *conv1_w, const float *conv1_b, void *out, size_t out_bytes, float *scale);
size_t srlhip_encoder_pack_bytes(void);
/* Host-only: layer 1 of the fused 64x64x3 kernel as it runs since round 6 — on the INT8 matrix pipe, exactly.  out = [channel half]
 * [kernel row 0..6][digit 0..2][lane][16 i8] (srlhip_encoder_pack_i8_bytes() bytes): the folded weight of output channel o at k =
 * row * 32 + slot * 4 + c (zero_slot = 0, the fused kernel: slot 0 empty, slot s = kernel column s - 1; zero_slot = 7, the layered
 * kernels of 3-channel frames of any other size: slot s = kernel column s, slot 7 empty; c < 3 the colour taps w / (255 std_c) that multiply p - 128,
 * c = 3 the validity-mask tap [sum_c w_c (128 / 255 - mean_c) / std_c plus the folded bias on the centre tap] / 127: the mask
 * byte of an inside pixel is 127) is the 24-bit
 * fixed-point number (65536 d0 + 256 d1 + d2) / scale_o with balanced digits d in [-128, 127]; inv_scale64[o] = 256 / scale_o, a
 * power of two.  Lane (h, n) of a fragment holds k = 16 h .. 16 h + 15 of output channel 32 * half + n. */
size_t srlhip_encoder_pack_i8_bytes(void);
int srlhip_encoder_pack_i8(const float *conv1_w, const float *conv1_b, int32_t zero_slot, void *out, size_t out_bytes, float *inv_scale64);
/* Host-only: the MFMA B-operand image create() uploads (normalisation folded into layer 1, every weight split
 * into f16 hi/lo), srlhip_encoder_pack_bytes() bytes.  Exposed so the packing can be checked without a GPU. */
int srlhip_encoder_pack(const float *conv1_w, const float *conv1_b, const float *conv2_w, const float *conv3_w,
                        void *out, size_t out_bytes, float *scales3 /* power-of-two pre-scale of layers 1..3 */);

/* ---- PCA state baseline (raw_pixels -> state) -----------------------------------------------------------
 * Replaces SRLPCA.getState (state_representation/models.py:196-217: a pickled sklearn PCA applied on the host to one
 * flattened uint8 observation at a time, `self.model.transform(observation.reshape(-1, n_features))`) for a whole
 * DEVICE-resident batch of frames, as one launch.  The caller folds the model: w is [F][S] float64 =
 * components_.T (each column divided by sqrt(explained_variance_) when the PCA whitens), b is [S] = -(mean_ @ w);
 * F = H W C flattened in the frame's own order, 1 <= S <= 64, F >= 1 (srlhip_pca_supported() tells beforehand; anything
 * else -> SRLHIP_ENOTSUP and the caller keeps the PyTorch formulation).
 * THE ARITHMETIC (csrc/pca_project.hpp, one text for the kernel, the host twin and the host check program): the
 * features f = 0 .. F - 1 are cut into chunks of 512 (the last one ragged); a chunk's sum starts from +0.0 and takes its
 * features in ascending order, acc = fma((double) x[i][f], w[f][s], acc) — the byte as it lies, no / 255; the state is the
 * chunks' sums added in ascending chunk order, starting with chunk 0's, then b[s]; with states_f32 the float64 state is
 * rounded once to float32.  The order depends on F alone: a frame's state does not depend on n, on its place in the
 * batch or on the launch's shape, and two forwards of the same input give the same bits.  Against an exactly rounded
 * reference every element is within (F + chunks + 1) 2^-52 (sum_f x_f |w_fs| + |b_s|).
 * srlhip_pca_forward: images_dev uint8 [n][F] and states_dev [n][S] (float64, or float32 with states_f32 = 1) are DEVICE
 * pointers on device_id; the call only enqueues on hip_stream (NULL = the default stream); n = 0 succeeds and launches
 * nothing.  The handle keeps grow-only scratch (the chunk sums of a launch, at most 512 MiB or one frame tile's: a larger
 * batch goes as several launches, one behind the other) PER STREAM it has been given: forwards on one stream are ordered
 * and share it, forwards on different streams of one handle may overlap.  A caller that captures the forward into a HIP
 * graph calls it once with its batch size, on the stream it captures, before capturing; the captured forward uses that
 * stream's scratch, so replays run on that stream, or ordered against its other forwards.  One host thread at a time
 * calls into a handle.
 * srlhip_pca_project_host is the host twin (host pointers, no GPU): the same header functions, the same bits — to this
 * contract what srlhip_jpeg_encode_host is to the JPEG one.  Without a GPU srlhip_pca_create fails with SRLHIP_EHIP and
 * a message (srlhip_pca_last_error(NULL)). */
typedef struct srlhip_pca *srlhip_pca_handle;
int srlhip_pca_supported(int64_t n_features, int32_t state_dim);              /* host only */
int srlhip_pca_create(int32_t device_id, int64_t n_features, int32_t state_dim,
                      const double *w /* [F][S] */, const double *b /* [S] */, srlhip_pca_handle *out);
int srlhip_pca_forward(srlhip_pca_handle p, const uint8_t *images_dev, int32_t n,
                       void *states_dev, int32_t states_f32, void *hip_stream);  /* enqueue-only */
int srlhip_pca_project_host(int64_t n_features, int32_t state_dim, const double *w, const double *b,
                            const uint8_t *images, int32_t n, void *states, int32_t states_f32); /* host only */
int srlhip_pca_destroy(srlhip_pca_handle p);
const char *srlhip_pca_last_error(srlhip_pca_handle p);

/* ---- fitting the PCA baseline: the Gram matrix of recorded frames ----------------------------------------
 * The hot part of state_representation/pca_fit.py (the closed-form fit of the model the calls above apply).  frames is
 * uint8 [n][F] row-major, as srlhip_render leaves them:
 *     gram[i][j] = sum_f frames[i][f] frames[j][f]   int64 [n][n], full and symmetric
 *     rowsum[i]  = sum_f frames[i][f]                int64 [n]
 * EXACT integers: every summation order gives the same bits, so the device and the host twin agree bit for bit and the
 * result does not depend on split.  On the device (csrc/pca_gram.hip) one wavefront per 32 x 32 tile of the upper
 * triangle runs v_mfma_i32_32x32x32_i8 on the signed bytes x - 128 (gram = S + 128 (rowsum_i + rowsum_j) - 16384 F, padding
 * masked to a signed 0 after the xor, no byte outside [0, n F) read), an int32 accumulator takes at most 65536 features
 * before it is added into int64, and the K dimension is cut into slices over workgroups: split = 0 chooses their number,
 * split >= 1 asks for that many (slices that would be empty are not launched).  With one slice the plane is stored;
 * with several it is zeroed on the stream and every slice adds its share with 64-bit atomic adds.
 * Shapes: 1 <= n <= 8192, n_features >= 1, 2 n^2 n_features 65025 < 2^63 (which keeps the fit's integer centring in int64);
 * srlhip_pca_gram_supported tells beforehand, anything else -> SRLHIP_ENOTSUP.  A negative split or a null pointer ->
 * SRLHIP_EINVAL.  A refused call touches neither plane.  srlhip_pca_gram only enqueues on hip_stream (NULL = the default
 * stream): the zeroes (several slices), the row sums, the tiles, three kernels at most; all pointers are DEVICE pointers on device_id and
 * frames_dev needs no alignment (16-byte loads when it and n_features are multiples of 16, guarded bytes otherwise).
 * srlhip_pca_gram_host is the host twin (host pointers, plain int64 loops, no GPU).  The message of a failed call of
 * either is the calling thread's srlhip_pca_gram_last_error. */
int srlhip_pca_gram_supported(int32_t n, int64_t n_features);                 /* host only */
int srlhip_pca_gram(int32_t device_id, const uint8_t *frames_dev, int32_t n, int64_t n_features, int32_t split,
                    int64_t *gram_dev /* [n][n] */, int64_t *rowsum_dev /* [n] */, void *hip_stream);  /* enqueue-only */
int srlhip_pca_gram_host(const uint8_t *frames, int32_t n, int64_t n_features,
                         int64_t *gram, int64_t *rowsum);                     /* host only */
const char *srlhip_pca_gram_last_error(void);

/* ---- scoring a state representation: exact k nearest neighbours and the KNN-MSE terms ----------------------
 * What state_representation/evaluate.py measures a learned state space with (csrc/knn.hpp is the one text of the
 * arithmetic for the kernels of csrc/knn.hip, the host twin and the host check program).
 * INPUTS.  states [n][s] float64, or float32 with states_f32 = 1 (each value widened exactly to float64 on load).
 * queries int32 [q], indices into 0 .. n - 1, duplicates allowed; NULL means q = n and queries[i] = i (the q argument is
 * not read then).  ground truth optional, float64 [n][g].
 * DISTANCE.  For query row i and candidate j: diff_s = x[i][s] - x[j][s] in float64, d = fma(diff_s, diff_s, d) for
 * s = 0 .. S - 1 in ascending order from +0.0.  No Gram-trick expansion, no reassociation: d(i, j) and d(j, i) are the
 * same bits.
 * NEIGHBOURS.  The k neighbours of i are the k smallest elements of {(d(i, j), j) : j != i} under the total order
 * "smaller d first, then smaller j", listed ascending.  j == i is excluded by index, not by distance: a duplicate
 * state at another index is a legitimate neighbour at distance 0.  A candidate enters a list only through
 * d < worst || (d == worst && j < worst_j), so a NaN distance never enters (nor +inf: the empty slot is (-1, +inf)),
 * and a list that cannot be filled keeps (-1, +inf) in its tail.
 * OUTPUTS.  idx int32 [q][k], dist float64 [q][k].  With a ground truth, err float64 [q]: i = queries[r], e from +0.0,
 * n = 0 .. k - 1 outer and c = 0 .. g - 1 inner, t = gt[idx[r][n]][c] - gt[i][c], e = fma(t, t, e); err[r] = e / (double)k.
 * Slots with index -1 are skipped, the divisor stays k.  gt and err are both given or both NULL.
 * SHAPES.  2 <= n <= 2^20, 1 <= s <= 64, 1 <= k <= min(32, n - 1), 1 <= q <= 2^20, 1 <= g <= 32:
 * srlhip_knn_supported tells beforehand (g = 0: no ground truth), anything else -> SRLHIP_ENOTSUP.  A null required
 * pointer, a negative split, one of gt / err without the other, or — on the host twin — a query index outside
 * 0 .. n - 1 -> SRLHIP_EINVAL.  A refused call touches no output.  The order is total and every operation is an IEEE
 * float64 operation in a fixed sequence, so the result is unique: it does not depend on q, on a query's place in the
 * list, on the launch shape or on split, and the device equals the host twin bit for bit.
 * THE DEVICE CALL only enqueues on hip_stream (NULL = the default stream): one launch of partial lists over candidate
 * slices (split = 0 chooses their number, split >= 1 asks for that many, slices that would be empty are not launched)
 * and, with more than one slice, one launch that merges them.  It allocates nothing and presets nothing on the stream,
 * so it may be captured into a graph.  The partial lists live in workspace_dev: srlhip_knn_workspace_bytes(n, s, k, q,
 * split) bytes (0 = the shape is refused), 8-byte aligned, required also when one slice ends up being used.  All
 * pointers are DEVICE pointers on device_id; states need only their element's alignment.  The device call does not read
 * queries on the host: an index outside 0 .. n - 1 there neither reads nor writes out of bounds — its load is clamped
 * and its rows are (-1, +inf) (err 0). */
int srlhip_knn_supported(int32_t n, int32_t s, int32_t k, int32_t q, int32_t g);          /* host only; g = 0: no ground truth */
size_t srlhip_knn_workspace_bytes(int32_t n, int32_t s, int32_t k, int32_t q, int32_t split);
int srlhip_knn(int32_t device_id, const void *states_dev, int32_t states_f32, int32_t n, int32_t s,
               const int32_t *queries_dev, int32_t q, int32_t k, const double *gt_dev, int32_t g, int32_t split,
               int32_t *idx_dev, double *dist_dev, double *err_dev, void *workspace_dev, void *hip_stream);   /* enqueue-only */
int srlhip_knn_host(const void *states, int32_t states_f32, int32_t n, int32_t s, const int32_t *queries, int32_t q,
                    int32_t k, const double *gt, int32_t g, int32_t *idx, double *dist, double *err);          /* host only */
const char *srlhip_knn_last_error(void);                                                  /* the calling thread's */

/* ---- the trainable linear state encoder: forward, and gradient + Adam in one launch ----------------------------------
 * state = fc(flatten(preprocess(frame))): srl_zoo's `--model-type linear` [srl_zoo is an empty submodule of the
 * reference checkout: recalled, UNVERIFIED].  What state_representation/linear_srl.py trains with (csrc/linear_srl.hpp
 * is the one text of the arithmetic for the kernels of csrc/linear_srl.hip, the host twins and the host check program).
 * SHAPES: frames uint8 [n][F], flattened NHWC as srlhip_render leaves them; feature f belongs to channel f mod C;
 * V [F][S], m [F][S], v [F][S], c [S], G [n][S], states [n][S], all float64.  F >= 1, 1 <= S <= 64, 1 <= C <= 8
 * (srlhip_linear_srl_supported tells beforehand, anything else -> SRLHIP_ENOTSUP), 1 <= n <= 1024 (n < 1 -> SRLHIP_EINVAL,
 * n > 1024 -> SRLHIP_ENOTSUP).  scale [C] and offset [C] are HOST tables, read during the call: the caller passes
 * 1 / (255 std) and mean / std.  A null pointer, a table entry that is not finite, an lr that is not finite, a beta
 * outside [0, 1), a negative or non-finite eps, a bias correction outside (0, 1], a workspace that is null or not
 * 16-byte aligned -> SRLHIP_EINVAL.  A refused call touches nothing; its message is the calling thread's
 * srlhip_linear_srl_last_error.
 * THE ARITHMETIC, every operation an IEEE float64 operation in a fixed sequence:
 *   xn       = fma(scale[ch], (double) x, -offset[ch])                                   (fused)
 *   forward    the order of srlhip_pca_forward with xn in the byte's place: chunks of 512 features, within a chunk
 *              ascending acc = fma(xn, V[f][s], acc) from +0.0 (fused); the chunk sums added in ascending chunk
 *              order starting with chunk 0's, then + c[s] (separate additions).  A function of F alone.
 *   gradient   g[f][s] from +0.0, for i = 0 .. n - 1 ascending g = fma(xn[i][f], G[i][s], g) (fused).  No atomics and
 *              no split over i: a function of n alone, not of the launch shape.
 *   Adam       every operation SEPARATE, division and square root correctly rounded; the caller passes
 *              bc1 = 1 - beta1^t and bc2 = 1 - beta2^t:
 *                m = (beta1 * m) + ((1 - beta1) * g)
 *                v = (beta2 * v) + (((1 - beta2) * g) * g)
 *                V = V - ((lr / bc1) * (m / ((sqrt(v) / sqrt(bc2)) + eps)))
 * so the device equals the host twin bit for bit, in the states, in grad_out and in V, m, v after any number of steps.
 * THE DEVICE CALLS only enqueue on hip_stream (NULL = the default stream), allocate nothing and preset nothing: they
 * may be captured into a graph.  srlhip_linear_srl_forward is two launches (chunk sums into workspace_dev:
 * srlhip_linear_srl_workspace_bytes(F, S, n) bytes, 0 = the shape is refused; then the join).
 * srlhip_linear_srl_step is ONE launch that forms g and updates V, m, v in place; with a non-null grad_out_dev g is
 * also stored [F][S].  c and the loss heads are the caller's.  All pointers but the tables are DEVICE pointers on
 * device_id; the *_host twins take host pointers and need no GPU. */
int srlhip_linear_srl_supported(int64_t n_features, int32_t state_dim, int32_t n_channels);    /* host only */
size_t srlhip_linear_srl_workspace_bytes(int64_t n_features, int32_t state_dim, int32_t n);
int srlhip_linear_srl_forward(int32_t device_id, const uint8_t *frames_dev, int32_t n, int64_t n_features, int32_t state_dim,
                              int32_t n_channels, const double *scale, const double *offset, const double *v_dev,
                              const double *c_dev, double *states_dev, void *workspace_dev, void *hip_stream);   /* enqueue-only */
int srlhip_linear_srl_step(int32_t device_id, const uint8_t *frames_dev, int32_t n, int64_t n_features, int32_t state_dim,
                           int32_t n_channels, const double *scale, const double *offset, const double *g_dev, double *v_dev,
                           double *m_dev, double *v2_dev, double lr, double beta1, double beta2, double eps, double bc1,
                           double bc2, double *grad_out_dev, void *hip_stream);                                  /* enqueue-only */
int srlhip_linear_srl_forward_host(const uint8_t *frames, int32_t n, int64_t n_features, int32_t state_dim, int32_t n_channels,
                                   const double *scale, const double *offset, const double *v, const double *c,
                                   double *states);                                                            /* host only */
int srlhip_linear_srl_step_host(const uint8_t *frames, int32_t n, int64_t n_features, int32_t state_dim, int32_t n_channels,
                                const double *scale, const double *offset, const double *g, double *v, double *m,
                                double *v2, double lr, double beta1, double beta2, double eps, double bc1, double bc2,
                                double *grad_out);                                                             /* host only */
const char *srlhip_linear_srl_last_error(void);                                               /* the calling thread's */


#ifdef __cplusplus
}
#endif
#endif /* SRLHIP_H */
