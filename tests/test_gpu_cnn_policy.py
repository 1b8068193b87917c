"""srlhip_cnn_policy_act on the GPU: the scores (score_out) against the float64 restatement tests/cnn_policy_ref.py within 4 x E32 and
against the stand-alone host program cnn_policy_hostcheck BIT FOR BIT (csrc/cnn_policy.hpp is built with -ffp-contract=off on both
sides), the actions by the selection rule on the kernel's own score bits, the frozen plane, shards, and the action-stream counter."""
import numpy as np
import pytest

import cnn_policy_ref as ref
import mlp_sample_ref as msr

pytestmark = pytest.mark.gpu
CASES = ref.cases()
ENV_OF_A = {4: "MobileRobotGymEnv-v0", 6: "KukaButtonGymEnv-v0", 2: "MobileRobotGymEnv-v0", 3: "KukaButtonGymEnv-v0"}
SEED = 17


def make_env(H, W, C, n, A, discrete=True, first_env_id=0):
    from srlhip.pixel_env import RawPixelVecEnv
    return RawPixelVecEnv(ENV_OF_A[A], n, seed=SEED, img_shape=(H, W), first_env_id=first_env_id,
                          env_kwargs={"is_discrete": discrete, "multi_view": C == 6})


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def act(env, frames, params, per_env=True, sample=False, freeze=False, done_prev=None, frozen=None):
    """one srlhip_cnn_policy_act call on device copies -> numpy {"act", "score", "frozen"}"""
    import torch
    n = env.num_envs
    A = env.h.num_actions if env.cfg.is_discrete else env.h.action_dim
    keep = [dev(frames), dev(np.asarray(params, dtype=np.float32))]
    out = torch.full(tuple(env.actions.shape), -7, dtype=env.actions.dtype, device="cuda")
    score = torch.zeros((n, A), dtype=torch.float32, device="cuda")
    fz = None if frozen is None else dev(frozen)
    dp = None if done_prev is None else dev(done_prev)
    env.h.cnn_policy_act(keep[0].data_ptr(), out.data_ptr(), keep[1].data_ptr(), per_env=per_env, freeze_after_done=freeze,
                         done_prev=None if dp is None else dp.data_ptr(), frozen=None if fz is None else fz.data_ptr(), sample=sample,
                         score_out=score.data_ptr())
    env.h.sync()
    return {"act": out.cpu().numpy(), "score": score.cpu().numpy(), "frozen": None if fz is None else fz.cpu().numpy()}


@pytest.fixture(scope="module")
def programs():
    ref.build_programs()
    return ref.PROGRAMS


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_scores_and_actions(programs, tmp_path, case):
    name, frames, params, A, per_env = case
    n, H, W, C = frames.shape
    s64 = ref.forward64_batch(params, frames, A, per_env)
    host = ref.run_program(programs[0], tmp_path, frames, params, A, per_env=per_env)
    env = make_env(H, W, C, n, A)
    try:
        assert env.cnn_param_count() == ref.param_count(C, H, W, A)
        got = act(env, frames, params, per_env)
        err = ref.rel_err(got["score"], s64)
        print(name, "kernel score error", err, "tolerance", ref.SCORE_TOL)
        assert err <= ref.SCORE_TOL
        assert np.array_equal(got["score"].view(np.uint32), host["score"].view(np.uint32))         # the host program's bits
        assert np.array_equal(got["act"], got["score"].astype(np.float64).argmax(axis=1)) and np.array_equal(got["act"], host["act"])
        # sampled: K calls use the blocks c0 .. c0 + K - 1 of every env's stream (c0 = 0 after create), as K steps of
        # srlhip_rollout_mlp_policy_sampled do (tests/mlp_sample_ref.py: draws)
        K = 3
        u = msr.draws(SEED + np.arange(n), 0, K)
        for k in range(K):
            smp = act(env, frames, params, per_env, sample=True)
            assert np.array_equal(smp["score"], got["score"])
            for e in range(n):
                assert ref.sample_accepts(smp["score"][e], u[k][e], int(smp["act"][e]), 0.0), (k, e)
        # the frame the env has just rendered
        img = env.reset()
        import torch
        torch.cuda.synchronize()
        rendered = img.cpu().numpy().copy()
        got_r = act(env, rendered, params, per_env)
        err_r = ref.rel_err(got_r["score"], ref.forward64_batch(params, rendered, A, per_env))
        print(name, "rendered frames: kernel score error", err_r)
        assert err_r <= ref.SCORE_TOL
    finally:
        env.close()
    # continuous action mode: the row of scores (A = the env's action_dim, the first rows of the same fc block shapes differ: new parameters)
    Ac = 3 if A == 6 else 2
    pc = ref.random_params(np.random.RandomState(5), C, H, W, Ac, n if per_env else 1)
    pc = pc if per_env else pc[0]
    env = make_env(H, W, C, n, Ac, discrete=False)
    try:
        got = act(env, frames, pc, per_env)
        assert ref.rel_err(got["score"], ref.forward64_batch(pc, frames, Ac, per_env)) <= ref.SCORE_TOL
        assert np.array_equal(got["act"], got["score"])
    finally:
        env.close()


def test_freeze_and_constant_frame(programs, tmp_path):
    frames, params, done_prev, frozen = ref.constant_case()
    n, A = 5, 6
    s64 = ref.forward64_batch(params, frames, A)
    host = ref.run_program(programs[0], tmp_path, frames, params, A, freeze=True, done_prev=done_prev, frozen=frozen)
    env = make_env(45, 51, 3, n, A)
    try:
        r = act(env, frames, params, freeze=True, done_prev=done_prev, frozen=frozen)
        off = act(env, frames, params, freeze=False, done_prev=done_prev, frozen=frozen)
        sampled = [act(env, frames, params, sample=True, freeze=True, frozen=r["frozen"]) for _ in range(2)]
        after = act(env, frames, params, sample=True)
    finally:
        env.close()
    # without freeze_after_done both planes are ignored: the frozen plane stays as it was, every env acts
    assert np.array_equal(off["frozen"], frozen) and np.array_equal(off["act"], off["score"].astype(np.float64).argmax(axis=1))
    # sampled: a frozen env draws too — after two calls with frozen envs every env's third call uses block 2 of its stream
    u = msr.draws(SEED + np.arange(n), 0, 3)
    for k, smp in enumerate(sampled + [after]):
        assert np.array_equal(smp["score"], r["score"])
        for e in range(n):
            if k < 2 and r["frozen"][e]:
                assert smp["act"][e] == -1
            else:
                assert ref.sample_accepts(smp["score"][e], u[k][e], int(smp["act"][e]), 0.0), (k, e)
    stale = [ref.sample_accepts(after["score"][e], u[0][e], int(after["act"][e]), 0.0) for e in range(n) if r["frozen"][e]]
    assert not all(stale), "the check must tell block 2 from block 0 for a frozen env"
    assert r["frozen"].tolist() == [0, 1, 1, 1, 0] and np.array_equal(r["act"], host["act"])
    assert np.array_equal(r["score"].view(np.uint32), host["score"].view(np.uint32))
    live = r["frozen"] == 0
    assert (r["act"][~live] == -1).all() and np.array_equal(r["act"][live], r["score"][live].astype(np.float64).argmax(axis=1))
    keep = np.arange(n) != 2
    assert ref.rel_err(r["score"][keep], s64[keep]) <= ref.SCORE_TOL
    err_c = ref.rel_err(r["score"][2], s64[2])
    print("constant frame: kernel score error", err_c, "tolerance", ref.SCORE_TOL_CONSTANT)
    assert err_c <= ref.SCORE_TOL_CONSTANT
    env = make_env(45, 51, 3, n, 3, discrete=False)
    try:
        pc = ref.random_params(np.random.RandomState(6), 3, 45, 51, 3, n)
        c = act(env, frames, pc, freeze=True, done_prev=done_prev, frozen=frozen)
    finally:
        env.close()
    assert np.isnan(c["act"][~live]).all() and np.array_equal(c["act"][live], c["score"][live])


def test_shards_agree_bit_for_bit():
    _, frames, params, A, _ = [c for c in CASES if c[0] == "signs 64x64"][0]
    whole = make_env(64, 64, 3, 4, A)
    parts = [make_env(64, 64, 3, 2, A, first_env_id=f) for f in (0, 2)]
    try:
        w = act(whole, frames, params, sample=True)
        p = [act(parts[i], frames[2 * i:2 * i + 2], params[2 * i:2 * i + 2], sample=True) for i in range(2)]
    finally:
        for e in [whole] + parts:
            e.close()
    assert np.array_equal(w["score"].view(np.uint32), np.concatenate([q["score"] for q in p]).view(np.uint32))
    assert np.array_equal(w["act"], np.concatenate([q["act"] for q in p]))


def test_refusals_on_a_handle():
    from srlhip import _lib
    import torch
    env = make_env(64, 64, 3, 2, 4)
    try:
        buf = torch.zeros((2, 64, 64, 3), dtype=torch.uint8, device="cuda")
        par = torch.zeros((2, env.cnn_param_count()), dtype=torch.float32, device="cuda")
        out = torch.zeros((2,), dtype=torch.int32, device="cuda")
        with pytest.raises(_lib.SrlHipError, match="frozen"):
            env.h.cnn_policy_act(buf.data_ptr(), out.data_ptr(), par.data_ptr(), freeze_after_done=True)
        with pytest.raises(_lib.SrlHipError, match="null images or act_out"):
            env.h.cnn_policy_act(None, out.data_ptr(), par.data_ptr())
    finally:
        env.close()
    cfg = _lib.default_config(_lib.ENV_MOBILE)
    cfg.num_envs, cfg.io_device, cfg.auto_reset, cfg.rng_mode = 2, 1, 1, _lib.RNG_PHILOX
    h = _lib.Handle(cfg)                               # ground-truth observations
    try:
        with pytest.raises(_lib.SrlHipError, match="raw_pixels"):
            h.cnn_policy_act(buf.data_ptr(), out.data_ptr(), par.data_ptr())
    finally:
        h.close()
