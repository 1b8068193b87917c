// kuka_tree_select.hpp — WHICH instantiation of the full-model rollout kernels steps a Kuka handle, as pure functions of the
// configuration: no HIP types, no handle, no environment reads (kuka_tree.hip reads the two overrides and passes them in).  The launchers
// (kuka_tree.hip; kuka_tree_kernels.hpp: tree_rollout_launch) turn the tuple chosen here into template arguments.  A stand-alone host
// program (kuka_tree_select_hostcheck.cpp, make treeselecthostcheck) prints both selectors over the whole configuration space, and
// tests/test_kuka_tree_select_cpu.py holds every line to an independent restatement of the rules.
#pragma once
#include "../../include/srlhip.h"

namespace srl {

enum TreeFamily {
    TREE_NONE = 0,      // (persistent selector only) the configuration has no persistent instantiation
    TREE_RB,            // KukaRandButtonGymEnv, free bodies:  kuka_tree_rollout_k<MODE, joints, given, 1, RB 1>        kuka_tree_rb.hip
    TREE_OCC,           // two wavefronts per SIMD:            kuka_tree_rollout_occ_k<MODE, given>                     kuka_tree_occ.hip
    TREE_SPEC,          // default configuration folded in:    kuka_tree_rollout_k<MODE, false, given, 1, 0, SPEC 1>    kuka_tree.hip
    TREE_GENERIC        // everything else:                    kuka_tree_rollout_k<MODE, joints, given, nb>             kuka_tree.hip
};
// family: TreeFamily; mode: SRLHIP_RNG_*; joints / given: 0 | 1; nb: buttons, 1 | 2; arm_signal: the launch carries the early completion
// signal of a single-step launch (step_signal.hpp).  The persistent selector returns the same tuple with given = 1, arm_signal = 0.
struct TreeSelect { int family, mode, joints, given, nb, arm_signal; };

inline bool tree_device_rng(const srlhip_config &c) { return c.rng_mode == SRLHIP_RNG_PHILOX || c.rng_mode == SRLHIP_RNG_MT19937; }
inline bool tree_joint_actions(const srlhip_config &c) { return !c.is_discrete && c.action_joints; }

// "This handle has the reference's default KukaButtonGymEnv configuration" (kuka_button_gym_env.py:93-98 ctor defaults: discrete
// actions, static button, force_down, sparse reward, action_repeat 1), auto-reset, a device RNG mode and the model table's default solver
// details: what kuka_tree_rollout_k<..., SPEC = 1> folds in as compile-time constants.  The observation mode is the caller's to test: the
// kernel folds in ground truth, which also serves a launch that writes no observation at all.
inline bool tree_spec_config(const srlhip_config &c, double solver_detail) {
    return solver_detail == 0.0 && c.env_kind == SRLHIP_ENV_KUKA_BUTTON && tree_device_rng(c) && c.is_discrete && !c.action_joints &&
           !c.random_target && c.force_down && !c.shape_reward && c.action_repeat == 1 && c.auto_reset;
}

// kuka_tree_launch on a full-model handle.  has_obs: an observation plane was passed; signal_ready: the host side armed the early
// completion signal (Handle::step_signal.done); occ_force: SRLHIP_KUKA_OCC, -1 unset, else whether it starts with '1'; spec_allowed:
// SRLHIP_KUKA_SPEC is unset or non-zero.
inline TreeSelect tree_select_launch(const srlhip_config &c, int n, bool given, int T, bool has_obs, double solver_detail, bool signal_ready,
                                     int occ_force, bool spec_allowed) {
    const int arm = signal_ready && T == 1 && given ? 1 : 0, g = given ? 1 : 0, joints = tree_joint_actions(c) ? 1 : 0;
    if (c.env_kind == SRLHIP_ENV_KUKA_RAND) return {TREE_RB, c.rng_mode, joints, g, 1, arm};       // never the OCC or SPEC form
    // raw_pixels without an observation plane: the rasteriser draws, the stepper writes no observation
    const bool spec = spec_allowed && tree_spec_config(c, solver_detail) &&
                      (c.obs_mode == SRLHIP_OBS_GROUND_TRUTH || (c.obs_mode == SRLHIP_OBS_RAW_PIXELS && !has_obs));
    // Very large batches run the two-wavefront kernel, but only configurations the specialised kernel does not cover: where that one
    // applies it is the faster one at every size measured (kuka_tree.hip has the figures).  A forced 1 wins over spec.
    const bool occ = occ_force >= 0 ? occ_force != 0 : (n >= 65536 && !spec);
    const bool one_button = c.env_kind == SRLHIP_ENV_KUKA_BUTTON || c.env_kind == SRLHIP_ENV_KUKA_MOVING;
    const bool cartesian = c.is_discrete || !c.action_joints;
    if (occ && one_button && cartesian) return {TREE_OCC, c.rng_mode, 0, g, 1, 0};                   // block 128, 8 envs per block, no signal
    if (spec) return {TREE_SPEC, c.rng_mode, 0, g, 1, arm};
    if (c.env_kind == SRLHIP_ENV_KUKA_2BUTTON) return {TREE_GENERIC, c.rng_mode, 0, g, 2, arm};     // Kuka2ButtonGymEnv takes discrete actions only: joints is ignored
    return {TREE_GENERIC, c.rng_mode, joints, g, 1, arm};
}

// The resident kernel of persistent stepping (srlhip_set_persistent): KukaButtonGymEnv, KukaMovingButtonGymEnv and Kuka2ButtonGymEnv on a
// device RNG mode — the specialised kernel where the configuration is the default one, the generic one otherwise (random_target, shaped
// reward, continuous Cartesian or joint-space actions, the joints observation modes, other solver details).  SRLHIP_KUKA_SPEC is NOT
// consulted here, and that is deliberate: the override exists for the tests that compare the two LAUNCHING forms, and persistent
// stepping has never honoured it.  (raw_pixels handles have no persistent form at all, so "ground truth" needs no second clause.)
inline TreeSelect tree_select_persist(const srlhip_config &c, double solver_detail) {
    const TreeSelect none = {TREE_NONE, c.rng_mode, 0, 0, 0, 0};
    if (c.kuka_model != SRLHIP_KUKA_MODEL_FULL || c.env_kind == SRLHIP_ENV_KUKA_RAND || !tree_device_rng(c) || c.obs_mode == SRLHIP_OBS_RAW_PIXELS)
        return none;
    if (c.env_kind == SRLHIP_ENV_KUKA_2BUTTON) return c.is_discrete ? TreeSelect{TREE_GENERIC, c.rng_mode, 0, 1, 2, 0} : none;
    if (tree_spec_config(c, solver_detail) && c.obs_mode == SRLHIP_OBS_GROUND_TRUTH) return {TREE_SPEC, c.rng_mode, 0, 1, 1, 0};
    return {TREE_GENERIC, c.rng_mode, tree_joint_actions(c) ? 1 : 0, 1, 1, 0};
}

}  // namespace srl
