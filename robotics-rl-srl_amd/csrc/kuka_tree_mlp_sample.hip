// kuka_tree_mlp_sample.hip — srlhip_rollout_mlp_policy_sampled on the full Kuka model: the four POLICY = 3 instantiations of
// kuka_tree_rollout_k (through kuka_tree_kernels.hpp's kuka_tree_policy_launch).  A translation unit of its own, as kuka_tree_mlp.hip:
// they spill as heavily and compile as slowly.
#include "kuka_tree_kernels.hpp"

namespace srl {
using namespace kuka;

int kuka_rollout_mlp_policy_sampled(Handle *h, int T, const PolicyArgs &pol, double *d_hdr, float *obs, float *d_rew, uint8_t *d_done, void *d_act_out, const SummaryOut *sum) {
    return kuka_tree_policy_launch<3>(h, sum ? kSummaryName : "rollout_mlp_policy_sampled", T, pol, d_hdr, obs, d_rew, d_done, d_act_out, sum);
}

}  // namespace srl
