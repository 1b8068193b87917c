// kuka_group.hip — lane-group Kuka rollout kernels for the baked model (see kuka_group.hpp / kuka_group_kernels.hpp).
#include "kuka_group_kernels.hpp"

namespace srl {
using namespace kuka;

int kuka_group_launch_baked(Handle *h, const KukaParams &p, int T, const void *d_actions, const double *d_noise, float *obs, float *d_rew,
                            uint8_t *d_done, void *d_act_out) {
    return group_rollout_launch<false>(h, p, T, d_actions, d_noise, obs, d_rew, d_done, d_act_out);
}

}  // namespace srl
