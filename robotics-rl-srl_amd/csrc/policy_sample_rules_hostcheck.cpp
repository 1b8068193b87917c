// policy_sample_rules_hostcheck.cpp — the rules of srlhip_rollout_policy_sampled and srlhip_sample_actions (api_rules.hpp:
// check_rollout_policy_sampled_config, check_sample_actions) as a stand-alone host program that prints their verdicts over their case
// space, one line per case: what tests/test_policy_sample_cpu.py checks line by line against the rules restated in Python.  A program of
// its own: api_rules_hostcheck's output stays what it was.  No HIP, no GPU (make policysampleruleshostcheck).
#include <stdio.h>

#include "api_rules.hpp"

using namespace srl;

static void verdict(const Verdict &v) { printf("%d %s\n", v.code, v.code ? v.msg : "-"); }

int main() {
    // srlhip_rollout_policy_sampled: the case space of api_rules_hostcheck's policy-config lines; beside each verdict, those of the
    // unsampled linear rollout and of the sampled MLP rollout on the same config
    for (int mode = 0; mode < 3; mode++) for (int ar = 0; ar < 2; ar++) for (int om = 0; om <= 3; om++)
    for (int kind : {SRLHIP_ENV_MOBILE, SRLHIP_ENV_MOBILE_1D, SRLHIP_ENV_KUKA_BUTTON, SRLHIP_ENV_KUKA_MOVING, SRLHIP_ENV_KUKA_2BUTTON, SRLHIP_ENV_KUKA_RAND})
    for (int km = 0; km < 2; km++) for (int disc = 0; disc < 2; disc++) {
        srlhip_config c;
        fill_default_config(kind, &c);
        c.rng_mode = mode; c.auto_reset = ar; c.obs_mode = om; c.kuka_model = km; c.is_discrete = disc;
        const Verdict s = check_rollout_policy_sampled_config(c), plain = check_rollout_policy_config(c, false), mlp = check_rollout_policy_config(c, true);
        printf("sampled-config %d %d %d %d %d %d | %d %d | ", mode, ar, om, kind, km, disc, plain.code, mlp.code);
        verdict(s);
    }
    // srlhip_sample_actions
    for (int scores = 0; scores < 2; scores++) for (int act = 0; act < 2; act++) for (int io = 0; io < 2; io++) for (int disc = 0; disc < 2; disc++)
    for (int kind : {SRLHIP_ENV_MOBILE_1D, SRLHIP_ENV_KUKA_RAND}) for (int om : {0, 3}) {
        srlhip_config c;
        fill_default_config(kind, &c);
        c.io_device = io; c.is_discrete = disc; c.obs_mode = om;
        printf("sample-actions %d %d %d %d %d %d | ", scores, act, io, disc, kind, om);
        verdict(check_sample_actions(c, scores != 0, act != 0));
    }
    return 0;
}
