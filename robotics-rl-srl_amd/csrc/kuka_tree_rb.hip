// kuka_tree_rb.hip — KukaRandButtonGymEnv on the full-model lane-group stepper: the RB = 1 instantiations of the rollout / reset kernels
// (kuka_tree_kernels.hpp), i.e. the arm + gripper tree with the env's eleven free bodies (ten distractors + the kicked ball,
// kuka_rand_button_gym_env.py:59-71,111-125) on lanes 0..10 — kuka_tree.hpp, free-body section.  A translation unit of its own so that it
// compiles beside kuka_tree.hip.
#include "kuka_tree_kernels.hpp"

namespace srl {
using namespace kuka;

int kuka_tree_rb_launch(Handle *h, const KukaParams &p, const TreeSelect &s, int T, const void *d_actions, const double *d_noise, float *obs, float *d_rew,
                        uint8_t *d_done, void *d_act_out) {
    const TreeIo io = {T, d_actions, d_noise, obs, d_rew, d_done, d_act_out};
    int rc = 0;
    const bool hit = dispatch_rollout_rng(s.mode, [&](auto mode) {
        return dispatch_int<0, 1>(s.joints, [&](auto joints) {
            return dispatch_int<0, 1>(s.given, [&](auto given) { rc = tree_rollout_launch<1>(h, p, mode, joints, given, Const<1>{}, s.arm_signal, io); });
        });
    });
    return hit ? rc : h->fail(SRLHIP_ENOTSUP, "rollout: no instantiation for this Kuka configuration");
}

int kuka_tree_rb_reset(Handle *h, const KukaParams &p, const uint8_t *d_mask, const double *d_host_rand, int stride, float *obs) {
    int rc = 0;
    const bool hit = dispatch_reset_rng(h->cfg.rng_mode, [&](auto mode) {
        return dispatch_int<0, 1>(tree_joint_actions(h->cfg) ? 1 : 0, [&](auto joints) {
            rc = tree_reset_launch<1>(h, p, mode, joints, Const<1>{}, d_mask, d_host_rand, stride, obs);
        });
    });
    return hit ? rc : h->fail(SRLHIP_ENOTSUP, "reset: no instantiation for this Kuka configuration");
}

}  // namespace srl
