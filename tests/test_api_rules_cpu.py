"""What the C-ABI front end decides from a config or from caller data (csrc/api_rules.hpp), without a GPU: the stand-alone host program
api_rules_hostcheck prints every rule over its case space — plain and under the address / undefined-behaviour sanitizers — and every line
is held to the rules restated here from the reference environments' definitions (cited as file:line of the reference's environments/
directory), not by calling the C++.  The header is then bound to the library: srlhip_default_config, and srlhip_create's refusals."""
import ctypes
import itertools

import numpy as np
import pytest

import api_rules_lines
from srlhip import _lib

EINVAL, ENOTSUP = -22, -95
MOBILE, MOBILE_1D, MOBILE_2TARGET, MOBILE_LINE, KUKA_BUTTON, KUKA_MOVING, KUKA_2BUTTON, KUKA_RAND = range(8)
GROUND_TRUTH, JOINTS, JOINTS_POSITION, RAW_PIXELS = range(4)
KINDS = range(8)
CONFIG_SIZE = 96                                         # sizeof(srlhip_config): 20 int32, an int64, a double


def is_mobile(kind):
    return 0 <= kind <= 3


def is_kuka(kind):
    return 4 <= kind <= 7


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
# (kinds outside the eight have no environment: check_config refuses them, and the shape functions answer as for "none of the listed
# kinds" — 0 observations, the MobileRobot defaults below 0 and the Kuka ones above 7, which is how their comparisons are written)
def obs_dim(kind, obs_mode):
    if kind == MOBILE_1D:
        return 1                                         # mobile_robot/mobile_robot_1D_env.py:50-51
    if is_mobile(kind):
        return 2                                         # mobile_robot/mobile_robot_env.py:152-153
    if is_kuka(kind):                                    # kuka_gym/kuka_button_gym_env.py:202-203, :199 (14 joints), :168 (both)
        return {JOINTS: 14, JOINTS_POSITION: 3 + 14}.get(obs_mode, 3)
    return 0


def num_actions(kind, disc):
    if not disc:
        return 0
    if kind == MOBILE_1D:
        return 2                                         # mobile_robot/mobile_robot_1D_env.py:3
    return 6 if is_kuka(kind) else 4                     # kuka_gym/kuka_button_gym_env.py:24, mobile_robot/mobile_robot_env.py:18


def action_dim(kind, disc, joints):
    if disc:
        return 1
    if kind >= KUKA_BUTTON:
        return 7 if joints else 3                        # kuka_gym/kuka_button_gym_env.py:154, :158
    return 2                                             # mobile_robot/mobile_robot_env.py:137


def frame_bytes(side_h, side_w, multi_view):
    return side_h * side_w * (6 if multi_view else 3)    # mobile_robot/mobile_robot_env.py:143; a second camera: three more channels


def reset_draws(kind, disc, random_target):
    if is_mobile(kind):
        start = 1 if kind == MOBILE_1D else 2            # mobile_robot_1D_env.py:66; mobile_robot_env.py:168-169
        target = {MOBILE: 2, MOBILE_1D: 1, MOBILE_LINE: 1, MOBILE_2TARGET: 4}[kind]      # mobile_robot_env.py:177-178, 1D:73, line_target:60, 2target:57-58 + 66-67
        return start + (target if random_target else 0)
    init = 10 if disc else 5                             # five initial actions: rand() + randint(3) each (kuka_button_gym_env.py:253-254), or one normal() (:259, :263)
    if kind == KUKA_2BUTTON:
        return (4 if random_target else 0) + 2 + init    # kuka_2button_gym_env.py:56-57, 67-68; :59-60 draws always
    return (1 if kind == KUKA_MOVING else 0) + (2 if random_target else 0) + (20 if kind == KUKA_RAND else 0) + init      # moving:40, button:230-231, rand_button:62-63 x 10


def config_verdict(kind, disc, obs_mode, rng_mode, auto_reset, kuka_model, info_bits, repeat, side_h, side_w, num_envs, struct_size=CONFIG_SIZE):
    """srlhip_create's refusals, in the order include/srlhip.h and the tests before this one pin"""
    if struct_size != CONFIG_SIZE:
        return EINVAL, "create: srlhip_config.struct_size mismatch (ABI)"
    if num_envs <= 0:
        return EINVAL, "create: num_envs must be positive"
    if not (is_mobile(kind) or is_kuka(kind)):
        return EINVAL, "create: unknown env_kind"
    if rng_mode not in (0, 1, 2):
        return EINVAL, "create: unknown rng_mode"
    if auto_reset and rng_mode == 0:
        return EINVAL, "create: auto_reset needs a device RNG mode"
    if not disc and kind in (MOBILE_1D, MOBILE_2TARGET):  # mobile_robot_1D_env.py:44, mobile_robot_2target_env.py:128-129 raise ValueError
        return ENOTSUP, "Only discrete actions is supported"
    if is_mobile(kind) and obs_mode not in (GROUND_TRUTH, RAW_PIXELS):
        return EINVAL, "create: MobileRobot envs support ground_truth / raw_pixels only"
    if not (8 <= side_h <= 1024 and 8 <= side_w <= 1024):
        return EINVAL, "create: img_h / img_w must be in [8, 1024]"
    if is_kuka(kind) and kuka_model not in (0, 1):
        return EINVAL, "create: unknown kuka_model"
    if info_bits not in (0, 1):
        return EINVAL, "create: info_bits must be 0 or 1"
    if is_kuka(kind) and repeat < 1:
        return EINVAL, "create: action_repeat must be >= 1"
    return 0, None


def show(verdict):
    return "{} {}".format(verdict[0], verdict[1] if verdict[0] else "-")


def default_fields(kind):
    """srlhip_default_config: the reference constructors' defaults"""
    max_distance, force_down = (0.8, 1) if is_kuka(kind) else (1.6, 1)
    if kind == KUKA_2BUTTON:
        max_distance, force_down = 2.0, 0                # kuka_gym/kuka_2button_gym_env.py:29
    return dict(struct_size=CONFIG_SIZE, env_kind=kind, num_envs=1, device_id=0, first_env_id=0, is_discrete=1, random_target=0, force_down=force_down,
                shape_reward=0, action_repeat=1, action_joints=0, obs_mode=GROUND_TRUTH, img_h=224, img_w=224, multi_view=0, rng_mode=2, auto_reset=1,
                io_device=0, kuka_model=1 if is_kuka(kind) else 0, info_bits=0, seed0=0, max_distance=max_distance)


CFG_SPACE = (range(-1, 9), (0, 1), range(0, 5), (0, 1), (0, 1), (0, 1), range(-1, 4), (0, 1), (0, 1, 2), (0, 1, 2), (0, 1), (7, 8, 1024, 1025), (0, 1))


def config_lines():
    for kind, disc, om, joints, rt, mv in itertools.product(*CFG_SPACE[:6]):
        od, na, ad = obs_dim(kind, om), num_actions(kind, disc), action_dim(kind, disc, joints)
        draws = reset_draws(kind, disc, rt) if is_mobile(kind) else reset_draws(KUKA_BUTTON if not is_kuka(kind) else kind, disc, rt)
        act = 3 * (4 if disc else 4 * ad)
        head = "cfg {} {} {} {} {} {} ".format(kind, disc, om, joints, rt, mv)
        for mode, ar, km, ib, rep, side, n in itertools.product(*CFG_SPACE[6:]):
            fb = frame_bytes(side, side, mv)
            yield "{}{} {} {} {} {} {} {} | {} {} {} {} {} {} {} {} | {}".format(
                head, mode, ar, km, ib, rep, side, n, od, na, ad, fb, fb if om == RAW_PIXELS else 4 * od, act, na if disc else ad, draws,
                show(config_verdict(kind, disc, om, mode, ar, km, ib, rep, side, side, n)))
    for h, w in ((7, 224), (1025, 224), (224, 7), (224, 1025)):
        yield "cfg-side {} {} | {}".format(h, w, show(config_verdict(MOBILE, 1, 0, 2, 1, 0, 0, 1, h, w, 1)))
    yield "cfg-size 4 | " + show(config_verdict(MOBILE, 1, 0, 2, 1, 0, 0, 1, 224, 224, 0, struct_size=4))


def pad16(x):
    return (x + 15) // 16 * 16


def layout(kind, disc, joints, om, side, mv, io, zc, n):
    """the host-pointer step's two buffers: [actions | pad | noise f64] in, [obs | pad | reward f32 | done u8] out; zero-copy when
    enabled, host pointers, no pixels and at most 1 MiB out"""
    pixels = om == RAW_PIXELS
    ob = n * (frame_bytes(side, side, mv) if pixels else 4 * obs_dim(kind, om))
    ab = n * (4 if disc else 4 * action_dim(kind, disc, joints))
    in_noise, out_rew = pad16(ab), pad16(ob)
    out_done = out_rew + 4 * n
    out_total = out_done + n
    return ob, ab, in_noise, in_noise + 8 * n, out_rew, out_done, out_total, int(pixels), int(bool(zc) and not io and not pixels and out_total <= 1 << 20)


def layout_lines():
    for kind, disc, joints, om, mv, io, zc, n in itertools.product(KINDS, (0, 1), (0, 1), range(4), (0, 1), (0, 1), (0, 1), (1, 3, 5, 4096)):
        yield "layout {} {} {} {} 8 {} {} {} {} | {}".format(kind, disc, joints, om, mv, io, zc, n, " ".join(map(str, layout(kind, disc, joints, om, 8, mv, io, zc, n))))
    # ground-truth MobileRobotGymEnv: out_total = pad16(8 n) + 5 n <= 2^20.  Without the padding n <= 2^20 / 13; the padding adds at most
    # 15 bytes, so the bound lies within two envs of that: walk down from above it
    n = (1 << 20) // 13 + 2
    while pad16(8 * n) + 5 * n > 1 << 20:
        n -= 1
    for m in (n, n + 1):
        out_total = pad16(8 * m) + 5 * m
        yield "bound {} | {} {}".format(m, out_total, int(out_total <= 1 << 20))


def caller_data_lines():
    # patterns of the middle row: 0 finite, 1 all NaN (the reference's None), 2 / 3 partly NaN, 4 / 5 an infinity, 6 NaNs and an infinity
    finite_all = {0: 1}
    kuka_ok = {0: 1, 1: 1}
    for dim, pattern in itertools.product((2, 3, 7), range(7)):
        yield "rows {} {} | {} {}".format(dim, pattern, finite_all.get(pattern, 0), kuka_ok.get(pattern, 0))
    for kind, joints, pattern in itertools.product((MOBILE, MOBILE_LINE, KUKA_BUTTON, KUKA_2BUTTON), (0, 1), range(7)):
        # MobileRobot's step indexes the action (mobile_robot_env.py:241-248: no None branch): finite rows only
        yield "actions {} {} {} | {}".format(kind, joints, pattern, (finite_all if is_mobile(kind) else kuka_ok).get(pattern, 0))
    for k in range(4):
        yield "noise {} | {}".format(k, int(k == 0))
    for top in (2, 4, 6):
        for value in (-2, -1, top - 1, top):             # -1: the reference's None action; the rest index a list of `top` entries
            yield "discrete {} {} | {} 0 {} {}".format(top, value, int(-1 <= value < top), value, top - 1)


TREE_HEADER = "set_kuka_tree_model: 12 DoFs, <= 16 spheres, end effector = link 6, max_generic_rows <= 6 (the lane group's row bank)"
TREE_JOINT = "set_kuka_tree_model: parents before children, positive masses / inertias / motor gains, unit axes"
TREE_ARM = "set_kuka_tree_model: DoFs 0..6 must be the serial arm"
TREE_SOLVER = "set_kuka_tree_model: solver_detail is a mask of SRLHIP_KUKA_DETAIL_* bits, erp values in [0, 1], linear_slop in [0, 0.01]"
TREE_SPHERE = "set_kuka_tree_model: bad sphere"
LUMPED = "set_kuka_model: masses and principal inertias must be positive, joint_lower < joint_upper"
# the program's cases in its order; None: accepted (a boundary value, or a field the check does not read)
MODEL_CASES = [("default", None)] + [(c, LUMPED) for c in ("mass0-zero", "mass6-negative", "mass3-nan", "inertia-x", "inertia-y", "inertia-z", "limits-equal",
                                                           "limits-swapped", "limits-nan")]
TREE_CASES = [("default", None), ("nd-11", TREE_HEADER), ("nd-13", TREE_HEADER), ("nsphere-negative", TREE_HEADER), ("nsphere-17", TREE_HEADER), ("nsphere-0", None),
              ("rows-negative", TREE_HEADER), ("rows-7", TREE_HEADER), ("rows-6", None), ("ee-link-5", TREE_HEADER), ("grip-link-negative", TREE_HEADER),
              ("grip-link-12", TREE_HEADER), ("parent-self", TREE_JOINT), ("parent-below-root", TREE_JOINT), ("mass-zero", TREE_JOINT), ("mass-nan", TREE_JOINT),
              ("inertia-xx", TREE_JOINT), ("inertia-yy", TREE_JOINT), ("inertia-zz", TREE_JOINT), ("axis-long", TREE_JOINT), ("axis-zero", TREE_JOINT),
              ("max-force-zero", TREE_JOINT), ("kp-negative", TREE_JOINT), ("arm-not-serial", TREE_ARM), ("gripper-reparented", None),
              ("two-clauses-joint-first", TREE_JOINT), ("two-clauses-header-first", TREE_HEADER), ("detail-half", TREE_SOLVER), ("detail-negative", TREE_SOLVER),
              ("detail-8", TREE_SOLVER), ("detail-7", None), ("contact-erp-negative", TREE_SOLVER), ("contact-erp-nan", TREE_SOLVER), ("limit-erp-high", TREE_SOLVER),
              ("slop-high", TREE_SOLVER), ("slop-negative", TREE_SOLVER), ("slop-top", None), ("sphere-link-negative", TREE_SPHERE), ("sphere-link-12", TREE_SPHERE),
              ("sphere-radius-zero", TREE_SPHERE), ("sphere-unused-bad", None), ("two-clauses-solver-first", TREE_SOLVER)]


def model_lines():
    for section, cases in (("model", MODEL_CASES), ("tree", TREE_CASES)):
        for name, msg in cases:
            yield "{} {} | {}".format(section, name, show((EINVAL, msg) if msg else (0, None)))


LINEAR_SIZE, MLP_SIZE = 48, 56                           # sizeof(srlhip_linear_policy), sizeof(srlhip_mlp_policy)


def first(*verdicts):
    return next((v for v in verdicts if v), (0, None))


def rollout_config_verdict(mode, ar, om, kind, km, disc, sample):
    """what has no fused policy kernel, in the order the entry points name it"""
    return first(mode == 0 and (ENOTSUP, "RNG_HOST is not supported (needs a device RNG mode)"),
                 not ar and (ENOTSUP, "needs auto_reset"),
                 om == RAW_PIXELS and (ENOTSUP, "raw_pixels observations are not supported (ground_truth only)"),
                 om == JOINTS and (ENOTSUP, "the joints observation mode is not supported (ground_truth only)"),
                 om == JOINTS_POSITION and (ENOTSUP, "the joints_position observation mode is not supported (ground_truth only)"),
                 kind == KUKA_RAND and (ENOTSUP, "KukaRandButtonGymEnv is not supported"),
                 is_kuka(kind) and km != 1 and (ENOTSUP, "the lumped Kuka model is not supported"),
                 sample and not disc and (ENOTSUP, "only discrete actions are sampled (the reference never samples continuous ones)"))


def policy_lines():
    yield "policy-abi linear null | " + show((EINVAL, "null policy"))
    yield "policy-abi mlp null | " + show((EINVAL, "null policy"))
    for name, own, sizes in (("linear", LINEAR_SIZE, (LINEAR_SIZE, LINEAR_SIZE - 8, MLP_SIZE, 0)), ("mlp", MLP_SIZE, (MLP_SIZE, MLP_SIZE + 8, LINEAR_SIZE, 0))):
        for size in sizes:
            yield "policy-abi {} {} | {}".format(name, size, show(first(size != own and (EINVAL, "srlhip_{}_policy.struct_size mismatch (ABI)".format(name)))))
    for hidden, reserved in itertools.product((-1, 0, 1, 100, 128, 129), (0, 1)):
        yield "policy-shape mlp {} {} | {}".format(hidden, reserved, show(first(not 1 <= hidden <= 128 and (EINVAL, "hidden must be in 1..128"),
                                                                                reserved != 0 and (EINVAL, "reserved must be 0"))))
    yield "policy-shape linear | 0 -"
    for what, w, norm, m, s in itertools.product(("weights", "params"), (0, 1), (0, 1), (0, 1), (0, 1)):
        yield "policy-pointers {} {} {} {} {} | {}".format(what, w, norm, m, s, show(first(not w and (EINVAL, "null " + what),
                                                                                         norm and not (m and s) and (EINVAL, "normalize needs obs_mean and obs_std"))))
    for kind, disc, joints, hidden in itertools.product(KINDS, (0, 1), (0, 1), (0, 1, 100)):
        D, A = obs_dim(kind, GROUND_TRUTH), num_actions(kind, disc) if disc else action_dim(kind, disc, joints)
        yield "policy-params {} {} {} {} | {}".format(kind, disc, joints, hidden, hidden * D + hidden + A * hidden + A if hidden else D * A)
    for mode, ar, om, kind, km, disc, sample in itertools.product((0, 1), (0, 1), range(4), (MOBILE, KUKA_BUTTON, KUKA_RAND), (0, 1), (0, 1), (0, 1)):
        yield "policy-config {} {} {} {} {} {} {} | {}".format(mode, ar, om, kind, km, disc, sample, show(rollout_config_verdict(mode, ar, om, kind, km, disc, sample)))
    # values: 0 fine, 1 NaN, 2 +inf; the std also 3 zero, 4 negative
    for what, norm, bw, bm, bs in itertools.product(("weights", "params"), (0, 1), range(3), range(3), range(5)):
        yield "policy-values {} {} {} {} {} | {}".format(what, norm, bw, bm, bs, show(first(bw and (EINVAL, "non-finite " + what),
                                                                                           norm and bm and (EINVAL, "non-finite obs_mean"),
                                                                                           norm and bs and (EINVAL, "obs_std entries must be finite and > 0"))))
    for l, m in itertools.product((0, 1), (0, 1)):
        yield "act-which {} {} | {}".format(l, m, show(first(l == m and (EINVAL, "pass exactly one of the linear and the MLP policy"))))
    for dim, sample, mlp in itertools.product((0, 1, 1024, 1025), (0, 1), (0, 1)):
        yield "act-shape {} {} {} | {}".format(dim, sample, mlp, show(first(not 1 <= dim <= 1024 and (EINVAL, "obs_dim must be in 1..1024"),
                                                                           sample and not mlp and (EINVAL, "only an MLP policy's actions are sampled"))))
    for obs, act, freeze, frozen, io, sample, disc in itertools.product(*[(0, 1)] * 7):
        yield "act-planes {} {} {} {} {} {} {} | {}".format(obs, act, freeze, frozen, io, sample, disc, show(first(
            not (obs and act) and (EINVAL, "null obs or act_out"), freeze and not frozen and (EINVAL, "freeze_after_done needs the frozen plane"),
            not io and (ENOTSUP, "device-pointer handles only (io_device = 1)"),
            sample and not disc and (ENOTSUP, "only discrete actions are sampled (the reference never samples continuous ones)"))))


def scratch_lines():
    for side, mv, n, blob_cap in itertools.product((8, 9, 224), (0, 1), (1, 5), (0, 1000, 65536)):
        ch = 6 if mv else 3
        ns = n * ch // 3                                 # one stream per camera
        cap = blob_cap // ns
        frames = pad16(side * (side + 8) * ch * n)
        ovf_at = frames + 8 * (ns + 1)                   # offsets: int64 [ns + 1]
        blob_at = pad16(ovf_at + 4 * ns)                 # overflow flags: int32 [ns]
        yield "jpeg {} {} {} {} | {} {} {} {} {} {} {} {} {}".format(side, mv, n, blob_cap, ch, ns, cap, frames, frames, ovf_at, blob_at, blob_at + cap * ns, frames)
    for n in (1, 3, 5, 4096):
        yield "episodes {} | {} 0 {}".format(n, 12 * n, 8 * n)       # float64 returns [n], then int32 lengths [n]


def default_lines():
    for kind in KINDS:
        f = default_fields(kind)
        yield "default {} | {} {:.17g}".format(kind, " ".join(str(f[name]) for name, _ in _lib.Config._fields_[:-1]), f["max_distance"])


def expected_lines():
    return itertools.chain(default_lines(), config_lines(), layout_lines(), caller_data_lines(), model_lines(), policy_lines(), scratch_lines())


@pytest.fixture(scope="module")
def built():
    api_rules_lines.build()


@pytest.fixture(scope="module", params=api_rules_lines.PROGRAMS)
def printed(request, built, tmp_path_factory):
    return api_rules_lines.run(request.param, tmp_path_factory.mktemp("rules"))


def test_every_line_follows_the_rules(printed):
    """both forms of the program print exactly the text the rules above give, line for line; the sanitized form ends clean"""
    count = 0
    with open(printed) as f:
        for want, got in itertools.zip_longest(expected_lines(), f):
            assert got is not None and got.rstrip("\n") == want, (count, want, got)
            count += 1
    assert count > 1000000


def test_default_models_pass_and_every_clause_is_broken_once(printed):
    v = api_rules_lines.verdicts(printed)
    assert v["model default"] == (0, None) and v["tree default"] == (0, None)
    refused = {msg for key, (code, msg) in v.items() if key.startswith(("model ", "tree ")) and code}
    assert refused == {LUMPED, TREE_HEADER, TREE_JOINT, TREE_ARM, TREE_SOLVER, TREE_SPHERE}


def test_default_config_is_the_headers(built):
    """srlhip_default_config, all eight kinds, field by field; a kind outside them is refused"""
    lib = _lib.load()
    for kind in KINDS:
        cfg = _lib.Config()
        assert lib.srlhip_default_config(kind, ctypes.byref(cfg)) == 0
        assert {name: getattr(cfg, name) for name, _ in _lib.Config._fields_} == default_fields(kind), kind
    for kind in (-1, 8):
        assert lib.srlhip_default_config(kind, ctypes.byref(_lib.Config())) == EINVAL
    assert ctypes.sizeof(_lib.Config) == CONFIG_SIZE and ctypes.sizeof(_lib.LinearPolicy) == LINEAR_SIZE and ctypes.sizeof(_lib.MlpPolicy) == MLP_SIZE


def test_create_refuses_what_the_header_refuses(built, tmp_path):
    """every refused config of the product: srlhip_create answers with the printed code and srlhip_last_error(NULL) with the printed
    message — before it touches a device.  (Accepted configs are not sent: they would open one.)"""
    lib = _lib.load()
    create, last_error = lib.srlhip_create, lib.srlhip_last_error
    cfg, h = _lib.default_config(MOBILE), ctypes.c_void_p()
    pc, ph = ctypes.byref(cfg), ctypes.byref(h)
    refused = 0
    with open(api_rules_lines.run("api_rules_hostcheck", tmp_path)) as f:
        for line in f:
            if not line.startswith("cfg "):
                continue
            inputs, _, verdict = line.rstrip("\n").split(" | ")
            code, _, msg = verdict.partition(" ")
            if code == "0":
                continue
            (cfg.env_kind, cfg.is_discrete, cfg.obs_mode, cfg.action_joints, cfg.random_target, cfg.multi_view, cfg.rng_mode, cfg.auto_reset, cfg.kuka_model,
             cfg.info_bits, cfg.action_repeat, side, cfg.num_envs) = map(int, inputs.split()[1:])
            cfg.img_h = cfg.img_w = side
            assert create(pc, ph) == int(code) and last_error(None) == msg.encode() and h.value is None, line
            refused += 1
    assert refused > 1000000
