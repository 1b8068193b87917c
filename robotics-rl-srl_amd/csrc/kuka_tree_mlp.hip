// kuka_tree_mlp.hip — srlhip_rollout_mlp_policy on the full Kuka model: the POLICY = 2 instantiations of kuka_tree_rollout_k
// (kuka_tree_kernels.hpp) — {PHILOX, MT19937} x {Cartesian one button, joint-space actions one button, Cartesian two buttons}, generic
// configuration (SPEC = 0), launching form — and the header kernel that hands the policy's scalars to them.  A translation unit of
// its own: kuka_tree_policy.hip and its code objects stay as they are.
#include "kuka_tree_kernels.hpp"

namespace srl {
using namespace kuka;

namespace {
// the 11 doubles the rollout kernel reads behind its `noise` argument (kuka_tree_policy.hip's ten, then the hidden width); a kernel,
// not a copy, for the same reason
__global__ void kuka_mlp_header_k(double *hdr, MlpPolicyArgs pol) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    hdr[0] = pol.per_env; hdr[1] = pol.freeze; hdr[2] = pol.normalize; hdr[3] = pol.clip;
    for (int d = 0; d < 3; d++) { hdr[4 + d] = pol.normalize ? pol.mean[d] : 0.0; hdr[7 + d] = pol.normalize ? pol.std[d] : 1.0; }
    hdr[10] = pol.hidden;
}
}  // namespace

int kuka_rollout_mlp_policy(Handle *h, int T, const MlpPolicyArgs &pol, double *d_hdr, float *obs, float *d_rew, uint8_t *d_done, void *d_act_out) {
    const srlhip_config &c = h->cfg;
    if (!h->kuka || !h->kuka->full || c.env_kind == SRLHIP_ENV_KUKA_RAND || c.obs_mode != SRLHIP_OBS_GROUND_TRUTH || !c.auto_reset ||
        (c.rng_mode != SRLHIP_RNG_PHILOX && c.rng_mode != SRLHIP_RNG_MT19937))
        return h->fail(SRLHIP_ENOTSUP, "rollout_mlp_policy: no policy instantiation for this Kuka configuration");
    // the two-button instantiation is JOINTS = false: it has six score rows, a joint-space policy has seven
    if (c.env_kind == SRLHIP_ENV_KUKA_2BUTTON && !c.is_discrete && c.action_joints)
        return h->fail(SRLHIP_ENOTSUP, "rollout_mlp_policy: Kuka2ButtonGymEnv with joint-space continuous actions is not supported");
    const KukaParams p = params_of(h);
    hipLaunchKernelGGL(kuka_mlp_header_k, dim3(1), dim3(64), 0, h->stream, d_hdr, pol);
    SRL_HIP_CHECK(h, hipGetLastError());
    dim3 grid(contiguous_grid((h->n + kGroupEnvs - 1) / kGroupEnvs)), block(kGroupBlock);      // as kuka_tree_launch: blocks map to envs XCD by XCD
    const bool joints = !c.is_discrete && c.action_joints, two = c.env_kind == SRLHIP_ENV_KUKA_2BUTTON;
    const void *d_w = pol.w;
    const double *hdr = d_hdr;
#define SRL_TREE_POL(MODE, J, NB) hipLaunchKernelGGL((kuka_tree_rollout_k<MODE, J, false, NB, 0, 0, 0, 2>), grid, block, 0, h->stream, p, *h->kuka, h->rng, h->stats, T, d_w, hdr, obs, d_rew, d_done, d_act_out, PersistArgs{})
#define SRL_TREE_POL_MODE(MODE)                       \
    if (two) SRL_TREE_POL(MODE, false, 2);            \
    else if (joints) SRL_TREE_POL(MODE, true, 1);     \
    else SRL_TREE_POL(MODE, false, 1);
    if (c.rng_mode == SRLHIP_RNG_PHILOX) { SRL_TREE_POL_MODE(SRLHIP_RNG_PHILOX) } else { SRL_TREE_POL_MODE(SRLHIP_RNG_MT19937) }
#undef SRL_TREE_POL_MODE
#undef SRL_TREE_POL
    SRL_HIP_CHECK(h, hipGetLastError());
    return 0;
}

}  // namespace srl
