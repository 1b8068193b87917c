"""CMA-ES from raw pixels on the device: RawPixelVecEnv.rollout_cnn_policy equals the hand-written loop of cnn_policy_act + step bit for
bit, CMAESModel trains with --cnn-policy per step and fused, a saved model replays the device's actions on host frames, and the
refusals around the flag stand."""
import argparse
import os

import numpy as np
import pytest

import cnn_policy_ref as ref

pytestmark = pytest.mark.gpu
IMG = (64, 64)


def host(planes):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in planes.items()}


@pytest.mark.parametrize("env_id,n,T", [("MobileRobotGymEnv-v0", 4, 6), ("KukaButtonGymEnv-v0", 3, 4)])
@pytest.mark.parametrize("sample", [False, True])
def test_rollout_equals_the_hand_written_loop(env_id, n, T, sample):
    """the planes of one enqueue-only rollout against a twin env driven call by call; from the step after an env's first done its
    action is -1"""
    import torch
    from srlhip.pixel_env import RawPixelVecEnv
    envs = [RawPixelVecEnv(env_id, n, seed=5, img_shape=IMG) for _ in range(2)]
    try:
        A = envs[0].h.num_actions
        params = torch.from_numpy(ref.random_params(np.random.RandomState(n + T), 3, 64, 64, A, n, "signs")).cuda()
        for e in envs:
            e.reset()
        got = host(envs[0].rollout_cnn_policy(T, params, per_env=True, freeze_after_done=True, sample=sample))
        twin, h = envs[1], envs[1].h
        frozen = torch.zeros((n,), dtype=torch.uint8, device="cuda")
        acts, rews, dones = [], [], []
        done_prev = None
        for t in range(T):
            a = torch.zeros((n,), dtype=torch.int32, device="cuda")
            h.cnn_policy_act(twin.images.data_ptr(), a.data_ptr(), params.data_ptr(), per_env=True, freeze_after_done=True,
                             done_prev=None if done_prev is None else done_prev.data_ptr(), frozen=frozen.data_ptr(), sample=sample)
            h.sync()
            _, r, d = twin.step(a)
            torch.cuda.synchronize()
            done_prev = d.clone()
            acts.append(a.cpu().numpy()); rews.append(r.cpu().numpy().copy()); dones.append(d.cpu().numpy().copy())
        assert np.array_equal(got["actions"], np.stack(acts))
        assert np.array_equal(got["reward"].view(np.uint32), np.stack(rews).view(np.uint32))
        assert np.array_equal(got["done"], np.stack(dones))
        seen = np.zeros(n, bool)
        for t in range(T):
            assert (got["actions"][t][seen] == -1).all() and (got["actions"][t][~seen] >= 0).all()
            seen |= (got["done"][t] & 1) != 0
    finally:
        for e in envs:
            e.close()


def test_frozen_envs_take_none_after_their_first_done():
    """MobileRobot episodes end after 250 steps at the latest: a rollout across that limit freezes every env"""
    import torch
    from srlhip.pixel_env import RawPixelVecEnv
    env = RawPixelVecEnv("MobileRobotGymEnv-v0", 2, seed=5, img_shape=(43, 43))
    try:
        params = torch.from_numpy(ref.random_params(np.random.RandomState(1), 3, 43, 43, 4, 1)[0]).cuda()
        env.reset()
        got = host(env.rollout_cnn_policy(256, params, per_env=False, freeze_after_done=True))
    finally:
        env.close()
    first = (got["done"] & 1).argmax(axis=0)
    assert ((got["done"] & 1).max(axis=0) == 1).all()
    for e in range(2):
        assert (got["actions"][:first[e] + 1, e] >= 0).all() and (got["actions"][first[e] + 1:, e] == -1).all()


def _args(**kw):
    base = dict(env="MobileRobotGymEnv-v0", seed=3, num_population=4, num_cpu=4, mu=0.0, sigma=0.14, num_timesteps=1, deterministic=True,
                continuous_actions=False, srl_model="raw_pixels", cnn_policy=True, num_stack=1, img_shape=(3,) + IMG, fused_rollout=False,
                fused_sampling=False, cuda=True, log_dir=None)
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.mark.parametrize("mode", ["per-step", "per-step sampled", "fused", "fused sampled"])
def test_training_save_load_and_replay(mode, tmp_path):
    import torch
    from rl_baselines.evolution_strategies.cma_es import BatchedCNN, CMAESModel
    from srlhip.pixel_env import RawPixelVecEnv
    fused, sampled = mode.startswith("fused"), mode.endswith("sampled")
    model = CMAESModel()
    # one generation of 4 members lives at most 4 x 251 steps: a budget of 1005 steps ends after the second generation at the latest
    model.train(_args(num_timesteps=1005, deterministic=not sampled, fused_rollout=fused, fused_sampling=fused and sampled))
    assert isinstance(model.policy, BatchedCNN) and model.policy.n_params == ref.param_count(3, 64, 64, 4) == len(model.best_model)
    assert 2 <= len(model.history) and np.isfinite(model.history).all()
    path = os.path.join(str(tmp_path), "cma.pkl")
    model.save(path)
    loaded = CMAESModel.load(path)
    assert isinstance(loaded.policy, BatchedCNN) and (loaded.policy.C, loaded.policy.img_h, loaded.policy.img_w, loaded.policy.A) == (3, 64, 64, 4)
    assert np.array_equal(loaded.best_model, model.best_model)
    if sampled:
        p = loaded.getActionProba(np.zeros((64, 64, 3), np.uint8))
        assert p.shape == (1, 4) and abs(p.sum() - 1.0) < 1e-9
        return
    # replay: the host forward of the saved model against the device action for the same parameters, wherever the float64 top-two gap
    # exceeds twice the score tolerance; at most one frame in twenty may be left out by that rule
    n = 20
    env = RawPixelVecEnv("MobileRobotGymEnv-v0", n, seed=11, img_shape=IMG)
    try:
        frames = env.reset()
        torch.cuda.synchronize()
        frames = frames.cpu().numpy().copy()
        params = torch.from_numpy(np.asarray(loaded.best_model, dtype=np.float32)).cuda()
        device = env.cnn_policy_act(params, per_env=False)
        torch.cuda.synchronize()
        device = device.cpu().numpy()
    finally:
        env.close()
    host_actions = loaded.getAction(frames)
    s64 = ref.forward64_batch(np.asarray(loaded.best_model, dtype=np.float32), frames, 4, per_env=False)
    top = np.sort(s64, axis=1)
    decided = (top[:, -1] - top[:, -2]) > 2 * ref.SCORE_TOL * np.maximum(1.0, np.abs(s64).max(axis=1))
    assert (~decided).sum() <= n // 20
    assert np.array_equal(host_actions[decided], device[decided])


def test_refusals():
    from rl_baselines.evolution_strategies.cma_es import CMAESModel
    with pytest.raises(NotImplementedError):
        CMAESModel.makeEnv(_args(cnn_policy=False, num_cpu=2))
    with pytest.raises(ValueError, match="num-stack"):
        CMAESModel.makeEnv(_args(num_stack=2, num_cpu=2))
    with pytest.raises(ValueError, match="num-stack"):
        CMAESModel().train(_args(num_stack=2))
