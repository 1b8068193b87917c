// kuka_tree_policy.hip — srlhip_rollout_policy on the full Kuka model: the POLICY = 1 instantiations of kuka_tree_rollout_k (through
// kuka_tree_kernels.hpp's kuka_tree_policy_launch), and the header kernel that hands a policy's scalars to them and to kuka_tree_mlp.hip's.
#include "kuka_tree_kernels.hpp"

namespace srl {
using namespace kuka;

namespace {
// the 11 doubles the rollout kernels read behind their `noise` argument (slot 10, the hidden width, by POLICY = 2 only); mean / std null
// without normalisation.  A kernel, not a copy: on device-pointer handles mean / std are device memory and the call may sit inside a
// stream capture.  Slots 11 .. 14 are not doubles: the four output pointers of srlhip_rollout_policy_summary as 64-bit words (all zero: the
// plane call) — the rollout kernel's own argument block stays the one every other instantiation shares.
__global__ void kuka_policy_hdr_k(double *hdr, PolicyArgs pol, SummaryOut sum) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    hdr[0] = pol.per_env; hdr[1] = pol.freeze; hdr[2] = pol.normalize; hdr[3] = pol.clip;
    for (int d = 0; d < 3; d++) { hdr[4 + d] = pol.normalize ? pol.mean[d] : 0.0; hdr[7 + d] = pol.normalize ? pol.std[d] : 1.0; }
    hdr[10] = pol.hidden;
    uint64_t *words = reinterpret_cast<uint64_t *>(hdr);
    words[11] = reinterpret_cast<uint64_t>(sum.ret); words[12] = reinterpret_cast<uint64_t>(sum.length);
    words[13] = reinterpret_cast<uint64_t>(sum.obs_sum); words[14] = reinterpret_cast<uint64_t>(sum.obs_sqsum);
}
}  // namespace

int kuka_policy_header(Handle *h, double *d_hdr, const PolicyArgs &pol, const SummaryOut *sum) {
    hipLaunchKernelGGL(kuka_policy_hdr_k, dim3(1), dim3(64), 0, h->stream, d_hdr, pol, sum ? *sum : SummaryOut{});
    SRL_HIP_CHECK(h, hipGetLastError());
    return 0;
}

int kuka_rollout_policy(Handle *h, int T, const PolicyArgs &pol, double *d_hdr, float *obs, float *d_rew, uint8_t *d_done, void *d_act_out, const SummaryOut *sum) {
    return kuka_tree_policy_launch<1>(h, sum ? kSummaryName : "rollout_policy", T, pol, d_hdr, obs, d_rew, d_done, d_act_out, sum);
}

}  // namespace srl
