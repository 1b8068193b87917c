"""srlhip_pixel_policy_act on the GPU: the scores (score_out) against the stand-alone host program pixel_policy_hostcheck and the numpy
restatement tests/pixel_policy_ref.py BIT FOR BIT (csrc/pixel_policy.hpp is built with -ffp-contract=off on both sides, and the summation
order is part of the contract), the actions by the selection rule on the kernel's own score bits, the frozen plane, shards, a launch
that walks its chunks in one workgroup against launches that split them, graph replay, and the refusals."""
import numpy as np
import pytest

import pixel_policy_ref as ref

pytestmark = pytest.mark.gpu
CASES = ref.cases()
SEED = 17


def make_env(H, W, C, n, A, discrete=True, first_env_id=0):
    from srlhip.pixel_env import RawPixelVecEnv
    return RawPixelVecEnv(ref.ENV_OF_A[(A, discrete)], n, seed=SEED, img_shape=(H, W), first_env_id=first_env_id,
                          env_kwargs={"is_discrete": discrete, "multi_view": C == 6})


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def act(env, frames, M, delta=None, noise=0.0, freeze=False, done_prev=None, frozen=None, graph_replays=0):
    """one srlhip_pixel_policy_act call on device copies -> numpy {"act", "score", "frozen"}; graph_replays: the call is captured and
    replayed that many times instead"""
    import torch
    n = env.num_envs
    A = env.h.num_actions if env.cfg.is_discrete else env.h.action_dim
    keep = [dev(frames), dev(M), None if delta is None else dev(delta)]
    out = torch.full(tuple(env.actions.shape), -7, dtype=env.actions.dtype, device="cuda")
    score = torch.full((n, A), 7.0, dtype=torch.float64, device="cuda")
    fz = None if frozen is None else dev(frozen)
    dp = None if done_prev is None else dev(done_prev)
    torch.cuda.synchronize()

    def call():
        env.h.pixel_policy_act(keep[0].data_ptr(), out.data_ptr(), keep[1].data_ptr(), delta=None if delta is None else keep[2].data_ptr(), noise=noise,
                               freeze_after_done=freeze, done_prev=None if dp is None else dp.data_ptr(), frozen=None if fz is None else fz.data_ptr(),
                               score_out=score.data_ptr())
    if graph_replays:
        env.h.graph_begin()
        call()
        g = env.h.graph_end()
        for _ in range(graph_replays):
            score.fill_(7.0)
            torch.cuda.synchronize()
            env.h.graph_launch(g)
            env.h.sync()
        env.h.graph_destroy(g)
    else:
        call()
    env.h.sync()
    return {"act": out.cpu().numpy(), "score": score.cpu().numpy(), "frozen": None if fz is None else fz.cpu().numpy()}


@pytest.fixture(scope="module")
def programs():
    ref.build_programs()
    return ref.PROGRAMS


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_scores_and_actions(programs, tmp_path, case):
    frames, M, delta, noise, A, discrete = (case[k] for k in ("frames", "M", "delta", "noise", "A", "discrete"))
    n, H, W, C = frames.shape
    want = ref.scores(frames, M, delta, noise)
    host = ref.run_program(programs[0], tmp_path, case)
    assert ref.same_bits(host["score"], want)
    env = make_env(H, W, C, n, A, discrete)
    try:
        got = act(env, frames, M, delta, noise)
        assert ref.same_bits(got["score"], want)                                   # paired = 1 with env 2k + 1 on its own frame; paired = 0
        # the selection on the kernel's own score bits: the strict argmax (numpy's: the first maximum) / the row (float)score
        assert ref.same_bits(got["act"], ref.select(got["score"], discrete)) and ref.same_bits(got["act"], host["act"])
        # the frame the env has just rendered
        import torch
        img = env.reset()
        torch.cuda.synchronize()
        rendered = img.cpu().numpy().copy()
        assert rendered.shape == frames.shape and rendered.max() > 0
        got_r = act(env, rendered, M, delta, noise)
        assert ref.same_bits(got_r["score"], ref.scores(rendered, M, delta, noise))
        live = env.pixel_policy_act(dev(M), None if delta is None else dev(delta), noise)     # the env's own method, on the frames where they lie
        torch.cuda.synchronize()
        assert ref.same_bits(live.cpu().numpy(), got_r["act"])
    finally:
        env.close()


@pytest.mark.parametrize("n,paired", [(512, True), (256, False)])
def test_one_workgroup_per_item_walks_the_chunks_in_the_same_order(n, paired):
    """45 x 51 x 3 is four chunks: below 256 work items every chunk has a workgroup of its own (the case list), from 256 on one
    workgroup walks them — the same bits, the restatement's"""
    H, W, C, A = 45, 51, 3, 4
    assert ref.chunks(H * W * C) == 4 and not ref.split(n // 2 if paired else n, H * W * C) and ref.split(5, H * W * C)
    rng = np.random.RandomState(n)
    frames = rng.randint(0, 256, size=(n, H, W, C)).astype(np.uint8)
    M = ref.mixed(rng, (H * W * C, A))
    delta = ref.mixed(rng, (n // 2, H * W * C, A)) if paired else None
    env = make_env(H, W, C, n, A)
    try:
        got = act(env, frames, M, delta, 0.37)
    finally:
        env.close()
    assert ref.same_bits(got["score"], ref.scores(frames, M, delta, 0.37))
    assert ref.same_bits(got["act"], ref.select(got["score"], True))


@pytest.mark.parametrize("A,discrete", [(6, True), (3, False), (2, False)])
def test_freeze_done_prev_and_the_frozen_plane(A, discrete):
    """-1, NaN rows on Kuka continuous, zero rows on MobileRobot continuous; bit 0 of done_prev alone counts"""
    case = [c for c in CASES if c["name"] == "45x51x3 A%d n10p" % A][0]
    done_prev = np.array([0, 1, 0, 3, 2, 0, 0, 1, 0, 0], np.uint8)
    frozen = np.array([0, 0, 1, 0, 0, 0, 1, 1, 0, 0], np.uint8)
    want_frozen = np.array([0, 1, 1, 1, 0, 0, 1, 1, 0, 0], np.uint8)
    env = make_env(45, 51, 3, 10, A, discrete)
    try:
        r = act(env, case["frames"], case["M"], case["delta"], case["noise"], freeze=True, done_prev=done_prev, frozen=frozen)
        plain = act(env, case["frames"], case["M"], case["delta"], case["noise"], freeze=True, frozen=np.zeros(10, np.uint8))
        off = act(env, case["frames"], case["M"], case["delta"], case["noise"], freeze=False, done_prev=done_prev, frozen=frozen)
    finally:
        env.close()
    want = ref.scores(case["frames"], case["M"], case["delta"], case["noise"])
    assert np.array_equal(r["frozen"], want_frozen) and ref.same_bits(r["score"], want)        # the scores stand as before the selection
    none_nan = A != 2                                      # A = 2: MobileRobot
    assert ref.same_bits(r["act"], ref.select(want, discrete, want_frozen, none_nan))
    gone = want_frozen != 0
    if discrete:
        assert (r["act"][gone] == -1).all()
    elif none_nan:
        assert np.isnan(r["act"][gone]).all()
    else:
        assert (r["act"][gone] == 0).all()
    assert not plain["frozen"].any() and ref.same_bits(plain["act"], ref.select(want, discrete))
    # without freeze_after_done both planes are ignored: the frozen plane stays as it was, every env acts
    assert np.array_equal(off["frozen"], frozen) and ref.same_bits(off["score"], want) and ref.same_bits(off["act"], ref.select(want, discrete))


def test_shards_agree_bit_for_bit():
    """a 10-env handle against two handles of 4 and 6 envs on the same frames and pair blocks"""
    case = [c for c in CASES if c["name"] == "45x51x3 A6 n10p"][0]
    whole = make_env(45, 51, 3, 10, 6)
    parts = [make_env(45, 51, 3, n, 6, first_env_id=f) for n, f in ((4, 0), (6, 4))]
    try:
        w = act(whole, case["frames"], case["M"], case["delta"], case["noise"])
        p = [act(parts[0], case["frames"][:4], case["M"], case["delta"][:2], case["noise"]),
             act(parts[1], case["frames"][4:], case["M"], case["delta"][2:], case["noise"])]
    finally:
        for e in [whole] + parts:
            e.close()
    assert ref.same_bits(w["score"], np.concatenate([q["score"] for q in p]))
    assert ref.same_bits(w["act"], np.concatenate([q["act"] for q in p]))


@pytest.mark.parametrize("name", ["8x8x3 A4 n5u", "45x51x3 A6 n10p"])      # one workgroup per item; a workgroup per chunk
def test_captured_call_replays_the_same_bits(name):
    case = [c for c in CASES if c["name"] == name][0]
    n, H, W, C = case["frames"].shape
    env = make_env(H, W, C, n, case["A"])
    try:
        direct = act(env, case["frames"], case["M"], case["delta"], case["noise"])
        replayed = act(env, case["frames"], case["M"], case["delta"], case["noise"], graph_replays=2)
    finally:
        env.close()
    assert ref.same_bits(direct["score"], replayed["score"]) and ref.same_bits(direct["act"], replayed["act"])
    assert ref.same_bits(direct["score"], ref.scores(case["frames"], case["M"], case["delta"], case["noise"]))


def test_refusals_on_a_handle():
    from srlhip import _lib
    import torch
    buf = torch.zeros((3, 8, 8, 3), dtype=torch.uint8, device="cuda")
    M = torch.zeros((192, 4), dtype=torch.float64, device="cuda")
    delta = torch.zeros((1, 192, 4), dtype=torch.float64, device="cuda")
    out = torch.zeros((3,), dtype=torch.int32, device="cuda")
    env = make_env(8, 8, 3, 3, 4)
    try:
        with pytest.raises(_lib.SrlHipError, match="even num_envs"):
            env.h.pixel_policy_act(buf.data_ptr(), out.data_ptr(), M.data_ptr(), delta=delta.data_ptr(), noise=0.1)
        with pytest.raises(_lib.SrlHipError, match="frozen"):
            env.h.pixel_policy_act(buf.data_ptr(), out.data_ptr(), M.data_ptr(), freeze_after_done=True)
        with pytest.raises(_lib.SrlHipError, match="null images or act_out"):
            env.h.pixel_policy_act(None, out.data_ptr(), M.data_ptr())
        env.h.pixel_policy_act(buf.data_ptr(), out.data_ptr(), M.data_ptr())          # unpaired: an odd num_envs is fine
        env.h.sync()
    finally:
        env.close()
    cfg = _lib.default_config(_lib.ENV_MOBILE)
    cfg.num_envs, cfg.io_device, cfg.auto_reset, cfg.rng_mode = 2, 1, 1, _lib.RNG_PHILOX
    h = _lib.Handle(cfg)                               # ground-truth observations
    try:
        with pytest.raises(_lib.SrlHipError, match="raw_pixels"):
            h.pixel_policy_act(buf.data_ptr(), out.data_ptr(), M.data_ptr())
    finally:
        h.close()
    cfg = _lib.default_config(_lib.ENV_MOBILE)
    cfg.num_envs, cfg.obs_mode, cfg.img_h, cfg.img_w = 2, _lib.OBS_RAW_PIXELS, 8, 8
    h = _lib.Handle(cfg)                               # host pointers
    try:
        with pytest.raises(_lib.SrlHipError, match="io_device"):
            h.pixel_policy_act(buf.data_ptr(), out.data_ptr(), M.data_ptr())
    finally:
        h.close()
