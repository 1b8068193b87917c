"""Policy rollouts on learned SRL states (PixelStateVecEnv.rollout_policy / rollout_mlp_policy: T x (srlhip_policy_act -> step + rasteriser
-> encoder) on one stream): the planes are what a twin env stepped through the public step() with the recorded actions produces, every
recorded action is the reference's choice for the recorded previous state, and ARS / CMA-ES train on a learned srl_model."""
import argparse

import numpy as np
import pytest

import mlp_policy_ref as ref
import mlp_sample_ref as msr
import policy_act_ref as par
import policy_exact as pe

pytestmark = pytest.mark.gpu
IMG = (64, 64)
_encoders = {}


def encoder(state_dim):
    import torch
    from state_representation.models import SRLNeuralNetwork
    if state_dim not in _encoders:
        torch.manual_seed(state_dim)
        _encoders[state_dim] = SRLNeuralNetwork(state_dim, cuda=True, img_shape=IMG)
    return _encoders[state_dim]


def make_env(env_id, n, state_dim, seed=5, discrete=True):
    from srlhip.pixel_env import PixelStateVecEnv
    return PixelStateVecEnv(env_id, n, encoder(state_dim), seed=seed, img_shape=IMG, env_kwargs={"is_discrete": discrete})


def host(planes):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in planes.items()}


def replay_on_twin(env_id, n, state_dim, actions, discrete=True, seed=5):
    """a twin env from the same seed, stepped through step() with the recorded actions -> (obs0, obs, reward, done)"""
    twin = make_env(env_id, n, state_dim, seed, discrete)
    obs0 = twin.reset().cpu().numpy().copy()
    obs, rew, done = [], [], []
    import torch
    for a in actions:
        s, r, d = twin.step(torch.from_numpy(np.ascontiguousarray(a)).cuda())
        torch.cuda.synchronize()
        obs.append(s.cpu().numpy().copy()); rew.append(r.cpu().numpy().copy()); done.append(d.cpu().numpy().copy())
    twin.close()
    return obs0, np.stack(obs), np.stack(rew), np.stack(done)


def check_rollout(env_id, n, T, state_dim, what, discrete=True, chunks=None, norm=None):
    import torch
    D = state_dim
    env = make_env(env_id, n, D, discrete=discrete)
    A = env.h.num_actions if discrete else env.h.action_dim
    none_nan = env_id.startswith("Kuka")
    H = 0 if what == "linear" else 17
    rng = np.random.RandomState(n + T + D)
    params = 0.5 * rng.standard_normal((n, D, A)) if not H else ref.random_params(7, (n, ref.param_count(D, H, A)))
    d_par = torch.from_numpy(params).cuda()
    stats = {}
    if norm is not None:
        stats = dict(obs_mean=torch.from_numpy(norm[0]).cuda(), obs_std=torch.from_numpy(norm[1]).cuda(), clip_obs=norm[2])
    env.reset()
    parts = []
    for t in (chunks or [T]):
        if H:
            parts.append(host(env.rollout_mlp_policy(t, d_par, H, freeze_after_done=chunks is None, sample=what == "sampled", **stats)))
        else:
            parts.append(host(env.rollout_policy(t, d_par, freeze_after_done=chunks is None, **stats)))
    env.close()
    out = {k: np.concatenate([p[k] for p in parts], 0) for k in parts[0]}
    # 1. a twin env reproduces the planes from the recorded actions: row pointers, stream order, auto-reset
    obs0, obs, rew, done = replay_on_twin(env_id, n, D, out["actions"], discrete)
    assert np.array_equal(pe.bits(out["obs"]), pe.bits(obs)) and np.array_equal(pe.bits(out["reward"]), pe.bits(rew))
    assert np.array_equal(out["done"], done)
    # 2. every recorded action is the reference's choice for the recorded previous state; frozen rows are `None`
    prev = np.concatenate([obs0[None], out["obs"][:-1]], 0)
    frozen = np.zeros(n, np.uint8)
    needed = live_total = 0
    u = msr.draws(5 + np.arange(n), 0, len(prev)) if what == "sampled" else None
    for t in range(len(prev)):
        kw = dict(params=params, hidden=H) if H else dict(weights=params)
        want = par.act(prev[t], D, A, discrete, freeze=chunks is None, done_prev=out["done"][t - 1] if t else None, frozen=frozen,
                       none_nan=none_nan, u=None if u is None else u[t], mean=None if norm is None else norm[0],
                       std=None if norm is None else norm[1], clip=10.0 if norm is None else norm[2], **kw)
        frozen = want["frozen"]
        live = want["live"]
        if what == "sampled":
            assert (out["actions"][t][~live] == -1).all()
            assert par.interval_ok(want["score"], u[t], out["actions"][t])[live].all()
            needed, live_total = needed + int((live & (out["actions"][t] != want["action"])).sum()), live_total + int(live.sum())
        else:
            assert np.array_equal(pe.bits(out["actions"][t]), pe.bits(want["action"])), t
    if what == "sampled":
        print("pixel sampled rollout: {} of {} live actions needed the interval rule".format(needed, live_total))
        assert needed <= pe.MAX_SHARE * live_total
    return out


@pytest.mark.parametrize("what", ["linear", "mlp", "sampled"])
def test_mobile_rollout_crosses_the_episode_end(what):
    out = check_rollout("MobileRobotGymEnv-v0", 5, 253, 3, what)
    assert out["done"].any() and (out["actions"][-1] == -1).all()


@pytest.mark.parametrize("n,state_dim,what,discrete", [(5, 3, "mlp", True), (70, 20, "mlp", True), (70, 3, "linear", True),
                                                      (5, 20, "sampled", True), (5, 3, "mlp", False)])
def test_kuka_rollout(n, state_dim, what, discrete):
    check_rollout("KukaButtonGymEnv-v0", n, 6, state_dim, what, discrete)


def test_chunked_calls_equal_one_call():
    one = check_rollout("KukaButtonGymEnv-v0", 5, 6, 3, "mlp")
    two = check_rollout("KukaButtonGymEnv-v0", 5, 6, 3, "mlp", chunks=[2, 4])
    for k in one:
        assert np.array_equal(pe.bits(one[k]) if one[k].dtype != np.uint8 else one[k], pe.bits(two[k]) if two[k].dtype != np.uint8 else two[k]), k


def test_frozen_statistics_reach_the_kernel_and_are_updated_once():
    import torch
    from srlhip.device_env import DeviceVecFrameStack, DeviceVecNormalize
    D, n, T, H = 3, 5, 6, 17
    mean, var = np.array([0.05, -0.02, 0.01]), np.array([0.011, 0.007, 0.013])
    base = make_env("KukaButtonGymEnv-v0", n, D)
    env = DeviceVecNormalize(DeviceVecFrameStack(base, 1), norm_obs=True, norm_reward=False, clip_obs=0.9)
    env.obs_rms.mean = torch.from_numpy(mean).cuda()
    env.obs_rms.var = torch.from_numpy(var).cuda()
    std = torch.sqrt(env.obs_rms.var + env.epsilon).cpu().numpy()          # what the wrapper hands to the kernel
    want = check_rollout("KukaButtonGymEnv-v0", n, T, D, "mlp", norm=(mean, std, 0.9))
    env.training = False
    env.reset()
    env.training = True
    count0 = float(env.obs_rms.count)
    A = base.h.num_actions
    params = torch.from_numpy(ref.random_params(7, (n, ref.param_count(D, H, A)))).cuda()
    got = host(env.rollout_mlp_policy(T, params, H, freeze_after_done=True))
    assert np.array_equal(got["actions"], want["actions"]) and np.array_equal(pe.bits(got["obs"]), pe.bits(want["obs"]))
    assert abs(float(env.obs_rms.count) - count0 - n * T) < 1e-6          # one update, from the T x n live rows
    with pytest.raises(NotImplementedError):
        DeviceVecFrameStack(base, 2).rollout_mlp_policy(T, params, H)
    env.close()


def _args(**kw):
    base = dict(env="MobileRobotGymEnv-v0", seed=3, srl_model="autoencoder", num_stack=1, log_dir=None, img_shape=IMG, state_dim=3,
                deterministic=True, continuous_actions=False, fused_rollout=False, fused_sampling=False, num_timesteps=4)
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.mark.parametrize("fused", [False, True])
def test_ars_trains_on_a_learned_srl_model(fused):
    import torch
    from rl_baselines.evolution_strategies.ars import ARSModel
    P = 2
    a = _args(num_population=P, top_population=2, step_size=0.02, exploration_noise=0.5, algo_type="v1", max_step_amplitude=10,
              num_cpu=2 * P, fused_rollout=fused)
    torch.manual_seed(0)                                 # the random-init encoder
    m = ARSModel().train(argparse.Namespace(**vars(a)))
    assert len(m.history) >= 1 and np.isfinite(m.history).all() and m.M.shape == (3, 4) and np.isfinite(m.M).all()
    if fused:                                            # the first evaluation again, by hand: same seed, same delta, M = 0
        torch.manual_seed(0)
        env = ARSModel.makeEnv(argparse.Namespace(**vars(a)))
        gen = torch.Generator(device=env.device)
        gen.manual_seed(a.seed)
        delta = torch.randn((P, 3, 4), dtype=torch.float64, device=env.device, generator=gen)
        model = ARSModel()
        model.exploration_noise = a.exploration_noise
        with torch.cuda.stream(env.torch_stream):
            env.reset()
            r, _ = model.evaluate_fused(env, torch.zeros((3, 4), dtype=torch.float64, device=env.device), delta, ARSModel.FUSED_EPISODE_LIMIT[0] + 1)
            again = float(r.mean())                      # (read on the env's stream)
        assert again == m.history[0]
        env.close()


@pytest.mark.parametrize("mode", ["per_step", "fused", "fused_sampling"])
def test_cma_es_trains_on_a_learned_srl_model(mode):
    import torch
    from rl_baselines.evolution_strategies.cma_es import CMAES, CMAESModel
    P = 4
    a = _args(num_population=P, mu=0.0, sigma=0.5, cuda=True, num_cpu=P, fused_rollout=mode != "per_step",
              fused_sampling=mode == "fused_sampling", deterministic=mode != "fused_sampling")
    torch.manual_seed(0)                                 # the random-init encoder
    m = CMAESModel().train(argparse.Namespace(**vars(a)))
    assert len(m.history) >= 1 and np.isfinite(m.history).all() and np.isfinite(m.best_model).all()
    if mode != "per_step":
        torch.manual_seed(0)
        env = CMAESModel.makeEnv(argparse.Namespace(**vars(a)))
        model = CMAESModel()
        model.policy, model.deterministic, model.continuous_actions = m.policy, m.deterministic, False
        population = CMAES(m.policy.n_params * [0.0], 0.5, P, env.device, seed=a.seed).ask()
        with torch.cuda.stream(env.torch_stream):
            env.reset()
            r, _ = model.evaluate_fused(env, population, CMAESModel.FUSED_EPISODE_LIMIT[0] + 1)
            again = float(r.mean())                      # (read on the env's stream)
        assert again == m.history[0]
        env.close()


def test_raw_pixels_and_ground_truth_are_as_before():
    from rl_baselines.evolution_strategies.cma_es import CMAESModel
    from srlhip.device_env import DeviceVecEnv
    with pytest.raises(NotImplementedError):
        CMAESModel.makeEnv(_args(srl_model="raw_pixels", num_cpu=2))
    env = CMAESModel.makeEnv(_args(srl_model="ground_truth", num_cpu=2))
    inner = env
    while hasattr(inner, "venv"):
        inner = inner.venv
    assert isinstance(inner, DeviceVecEnv)
    env.close()
