// kuka_tree_policy_sample.hip — srlhip_rollout_policy_sampled on the full Kuka model: the four POLICY = 4 instantiations of
// kuka_tree_rollout_k (through kuka_tree_kernels.hpp's kuka_tree_policy_launch): the linear policy's six scores, the draw of
// kuka_tree_mlp_sample.hip's kernels (row_softmax_draw).  A translation unit of its own, as that one: the kernels compile slowly.
#include "kuka_tree_kernels.hpp"

namespace srl {
using namespace kuka;

int kuka_rollout_policy_sampled(Handle *h, int T, const PolicyArgs &pol, double *d_hdr, float *obs, float *d_rew, uint8_t *d_done, void *d_act_out, const SummaryOut *sum) {
    return kuka_tree_policy_launch<4>(h, sum ? kSummaryName : "rollout_policy_sampled", T, pol, d_hdr, obs, d_rew, d_done, d_act_out, sum);
}

}  // namespace srl
