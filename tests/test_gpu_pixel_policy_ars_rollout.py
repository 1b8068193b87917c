"""ARS from raw pixels on the device: RawPixelVecEnv.rollout_pixel_policy equals the hand-written loop of pixel_policy_act + step bit for
bit and the reference's return accounting, ARSModel trains with --pixel-policy per step and fused to the same M, the sampling per-step
path draws valid actions, and the refusals around the flag stand."""
import argparse

import numpy as np
import pytest

import pixel_policy_ref as ref

pytestmark = pytest.mark.gpu
IMG = (16, 16)


def host(planes):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in planes.items()}


@pytest.mark.parametrize("env_id,pairs,T", [("MobileRobotGymEnv-v0", 4, 6), ("KukaButtonGymEnv-v0", 2, 4)])
@pytest.mark.parametrize("freeze", [False, True])
def test_rollout_equals_the_hand_written_loop(env_id, pairs, T, freeze):
    """the planes of one enqueue-only rollout against a twin env driven call by call"""
    import torch
    from srlhip.pixel_env import RawPixelVecEnv
    n = 2 * pairs
    envs = [RawPixelVecEnv(env_id, n, seed=5, img_shape=IMG) for _ in range(2)]
    try:
        A, D = envs[0].h.num_actions, IMG[0] * IMG[1] * 3
        rng = np.random.RandomState(n + T)
        M = torch.from_numpy(ref.mixed(rng, (D, A))).cuda()
        delta = torch.from_numpy(rng.normal(size=(pairs, D, A)) * 1e3).cuda()
        noise = 0.5
        for e in envs:
            e.reset()
        got = host(envs[0].rollout_pixel_policy(T, M, delta, noise, freeze_after_done=freeze))
        twin, h = envs[1], envs[1].h
        frozen = torch.zeros((n,), dtype=torch.uint8, device="cuda")
        acts, rews, dones, frames = [], [], [], []
        done_prev = None
        for t in range(T):
            a = torch.zeros((n,), dtype=torch.int32, device="cuda")
            frames.append(twin.images.cpu().numpy().copy())
            h.pixel_policy_act(twin.images.data_ptr(), a.data_ptr(), M.data_ptr(), delta=delta.data_ptr(), noise=noise, freeze_after_done=freeze,
                               done_prev=None if done_prev is None else done_prev.data_ptr(), frozen=frozen.data_ptr())
            h.sync()
            _, r, d = twin.step(a)
            torch.cuda.synchronize()
            done_prev = d.clone()
            acts.append(a.cpu().numpy()); rews.append(r.cpu().numpy().copy()); dones.append(d.cpu().numpy().copy())
        assert np.array_equal(got["actions"], np.stack(acts))
        assert np.array_equal(got["reward"].view(np.uint32), np.stack(rews).view(np.uint32))
        assert np.array_equal(got["done"], np.stack(dones))
        # every live action is the restatement's on the frame the env held, and the directions differ somewhere
        seen = np.zeros(n, bool)
        for t in range(T):
            want = ref.select(ref.scores(frames[t], M.cpu().numpy(), delta.cpu().numpy(), noise), True, seen if freeze else None)
            assert np.array_equal(got["actions"][t], want)
            seen |= (got["done"][t] & 1) != 0
        if freeze:
            from rl_baselines.evolution_strategies.ars import ARSModel
            ret, live_rows = ARSModel.returns_from_planes(torch.from_numpy(got["reward"]), torch.from_numpy(got["done"]))
            # the reference's accounting (ars.py:168-180): a direction's reward counts until it has reported done, the reporting step excluded
            want_ret, gone = np.zeros(n), np.zeros(n, bool)
            for t in range(T):
                gone |= (got["done"][t] & 1) != 0
                want_ret += got["reward"][t].astype(np.float64) * ~gone
            assert np.array_equal(ret.numpy(), want_ret) and 1 <= int(live_rows) <= T
    finally:
        for e in envs:
            e.close()


def _args(**kw):
    base = dict(env="MobileRobotGymEnv-v0", seed=3, num_population=4, top_population=2, step_size=0.02, exploration_noise=0.02, algo_type="v1",
                max_step_amplitude=10, num_cpu=8, num_timesteps=3000, deterministic=True, continuous_actions=False, srl_model="raw_pixels",
                pixel_policy=True, num_stack=1, img_shape=(3,) + IMG, fused_rollout=False, log_dir=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_fused_and_per_step_learners_end_with_the_same_M():
    """P = 4, 16 x 16 frames; an update advances the step count by 4 x 251, num_updates = 3000 // 4 * 2 = 1500: exactly two updates.  Both
    paths select through the same kernel on the same frames and the same planes feed the same update: the same M, bit for bit"""
    from rl_baselines.evolution_strategies.ars import ARSModel
    per_step = ARSModel().train(_args())
    fused = ARSModel().train(_args(fused_rollout=True))
    assert len(per_step.history) == len(fused.history) == 2
    assert per_step.M.shape == (16 * 16 * 3, 4) and np.abs(fused.M).max() > 0
    assert ref.same_bits(per_step.M, fused.M) and per_step.history == fused.history
    # a saved model acts on host frames
    frames = np.random.RandomState(0).randint(0, 256, size=(5, 16, 16, 3)).astype(np.uint8)
    assert np.array_equal(fused.getAction(frames), (frames.reshape(5, -1).astype(np.float64) @ fused.M).argmax(axis=1))


def test_sampling_per_step_learner_trains_and_draws_valid_actions():
    from rl_baselines.evolution_strategies.ars import ARSModel
    drawn = []

    class Recording(ARSModel):
        @staticmethod
        def pixel_actions(env, M, delta, noise, done, *a, **k):
            out = ARSModel.pixel_actions(env, M, delta, noise, done, *a, **k)
            drawn.append((out.clone(), done.clone()))
            return out

    model = Recording().train(_args(deterministic=False))
    assert len(model.history) == 2 and np.isfinite(model.history).all() and np.isfinite(model.M).all()
    import torch
    torch.cuda.synchronize()
    acts = torch.stack([a for a, _ in drawn]).cpu().numpy()
    done = torch.stack([d for _, d in drawn]).cpu().numpy()
    assert acts.dtype == np.int32 and (acts[done] == -1).all() and (acts[~done] >= 0).all() and (acts[~done] < 4).all()
    assert len(np.unique(acts[~done])) > 1


def test_refusals():
    from rl_baselines.evolution_strategies.ars import ARSModel
    with pytest.raises(NotImplementedError):
        ARSModel.makeEnv(_args(pixel_policy=False))
    with pytest.raises(ValueError, match="num-stack"):
        ARSModel.makeEnv(_args(num_stack=2))
    with pytest.raises(ValueError, match="num-stack"):
        ARSModel().train(_args(num_stack=2, fused_rollout=True))
