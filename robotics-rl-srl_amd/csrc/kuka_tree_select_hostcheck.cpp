// kuka_tree_select_hostcheck.cpp — the two selectors of kuka_tree_select.hpp over the whole configuration space, as a stand-alone host
// program that includes nothing else of the library.  TESTS ONLY (make treeselecthostcheck; tests/test_kuka_tree_select_cpu.py compares
// every line with its own restatement of the rules).  One fixed-width line per case on stdout:
//   EMDJRFSAPOV NNNNN GTBLCX|fmjgna|fmjgna
//   inputs   E env_kind  M rng_mode  D is_discrete  J action_joints  R random_target  F force_down  S shape_reward  A auto_reset
//            P action_repeat  O obs_mode  V solver_detail;  N num_envs;  G actions given  T steps  B observation plane passed
//            L early completion signal ready  C SRLHIP_KUKA_OCC (u unset, 0, 1)  X SRLHIP_KUKA_SPEC allows the specialised kernel
//   outputs  tree_select_launch, then tree_select_persist: family mode joints given nb arm_signal
#include <stdio.h>

#include "kuka_tree_select.hpp"

using namespace srl;

static char *put(char *o, const TreeSelect &s) {
    const int v[6] = {s.family, s.mode, s.joints, s.given, s.nb, s.arm_signal};
    *o++ = '|';
    for (int k = 0; k < 6; k++) *o++ = (char)('0' + v[k]);
    return o;
}

int main() {
    const int envs[4] = {SRLHIP_ENV_KUKA_BUTTON, SRLHIP_ENV_KUKA_MOVING, SRLHIP_ENV_KUKA_2BUTTON, SRLHIP_ENV_KUKA_RAND};
    const int modes[3] = {SRLHIP_RNG_HOST, SRLHIP_RNG_PHILOX, SRLHIP_RNG_MT19937};
    const int obs_modes[4] = {SRLHIP_OBS_GROUND_TRUTH, SRLHIP_OBS_JOINTS, SRLHIP_OBS_JOINTS_POSITION, SRLHIP_OBS_RAW_PIXELS};
    const int ns[3] = {4096, 65535, 65536};
    srlhip_config c = {};
    c.struct_size = (int32_t)sizeof c;
    c.kuka_model = SRLHIP_KUKA_MODEL_FULL;
    char line[64];
    for (int env : envs) for (int mode : modes) for (int disc = 0; disc < 2; disc++) for (int joints = 0; joints < 2; joints++)
    for (int rt = 0; rt < 2; rt++) for (int fd = 0; fd < 2; fd++) for (int sr = 0; sr < 2; sr++) for (int ar = 0; ar < 2; ar++)
    for (int rep = 1; rep <= 2; rep++) for (int om : obs_modes) for (int detail = 0; detail < 2; detail++) {
        c.env_kind = env; c.rng_mode = mode; c.is_discrete = disc; c.action_joints = joints; c.random_target = rt; c.force_down = fd;
        c.shape_reward = sr; c.auto_reset = ar; c.action_repeat = rep; c.obs_mode = om;
        const TreeSelect persist = tree_select_persist(c, (double)detail);
        for (int n : ns) {
        c.num_envs = n;
        char *const tail = line + snprintf(line, sizeof line, "%d%d%d%d%d%d%d%d%d%d%d %5d ", env, mode, disc, joints, rt, fd, sr, ar, rep, om, detail, n);
        for (int given = 0; given < 2; given++) for (int T = 1; T <= 2; T++) for (int has_obs = 0; has_obs < 2; has_obs++)
        for (int sig = 0; sig < 2; sig++) for (int occ = -1; occ <= 1; occ++) for (int spec_ok = 0; spec_ok < 2; spec_ok++) {
            const TreeSelect launch = tree_select_launch(c, n, given != 0, T, has_obs != 0, (double)detail, sig != 0, occ, spec_ok != 0);
            const char in[6] = {(char)('0' + given), (char)('0' + T), (char)('0' + has_obs), (char)('0' + sig), occ < 0 ? 'u' : (char)('0' + occ), (char)('0' + spec_ok)};
            char *o = tail;
            for (char ch : in) *o++ = ch;
            o = put(put(o, launch), persist);
            *o++ = '\n';
            if (fwrite(line, 1, (size_t)(o - line), stdout) != (size_t)(o - line)) return 2;
        }
        }
    }
    return fflush(stdout) == 0 ? 0 : 2;
}
