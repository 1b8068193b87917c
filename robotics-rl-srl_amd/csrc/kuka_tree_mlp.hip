// kuka_tree_mlp.hip — srlhip_rollout_mlp_policy on the full Kuka model: the POLICY = 2 instantiations of kuka_tree_rollout_k (through
// kuka_tree_kernels.hpp's kuka_tree_policy_launch).  A translation unit of its own: they spill heavily and compile slowly.
#include "kuka_tree_kernels.hpp"

namespace srl {
using namespace kuka;

int kuka_rollout_mlp_policy(Handle *h, int T, const PolicyArgs &pol, double *d_hdr, float *obs, float *d_rew, uint8_t *d_done, void *d_act_out, const SummaryOut *sum) {
    const srlhip_config &c = h->cfg;
    // the two-button instantiation is JOINTS = false: it has six score rows, a joint-space policy has seven.  (Ahead of the shared
    // launch's guard, which stood before it: that guard cannot fire for a call that came through the ABI — see there.)
    if (c.env_kind == SRLHIP_ENV_KUKA_2BUTTON && !c.is_discrete && c.action_joints)
        return h->fail(SRLHIP_ENOTSUP, std::string(sum ? kSummaryName : "rollout_mlp_policy") + ": Kuka2ButtonGymEnv with joint-space continuous actions is not supported");
    return kuka_tree_policy_launch<2>(h, sum ? kSummaryName : "rollout_mlp_policy", T, pol, d_hdr, obs, d_rew, d_done, d_act_out, sum);
}

}  // namespace srl
