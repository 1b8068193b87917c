"""Device-resident VecEnv stack: observations, rewards, dones and actions are torch tensors in HBM
(io_device = 1), so a policy that also lives on the GPU never round-trips through the host.

    DeviceVecEnv         the libsrlhip handle behind a tensor-in / tensor-out step()   (rl_baselines/utils.py:213-220)
    DeviceVecFrameStack  stable-baselines VecFrameStack on tensors                      (rl_baselines/utils.py:222)
    DeviceVecNormalize   stable-baselines VecNormalize (running mean / var) on tensors  (rl_baselines/utils.py:223-227)

Stream discipline: the handle owns a HIP stream (srlhip_stream).  `env.torch_stream` wraps it as a
torch.cuda.ExternalStream; code that runs under `with torch.cuda.stream(env.torch_stream):` is ordered with the
stepper's kernels and needs no host synchronisation at all.  When the caller is on another stream, step()/reset()
fall back to two host-side stream synchronisations per call."""
import contextlib
import functools

import numpy as np
import torch

from . import _lib
from .envs import ENV_CLASSES, OBS_MODES
from .gym_compat import Box, Discrete

from .vec_env import RNG_MODES, default_rng_mode


def _apply_env_kwargs(cfg, kw, int_keys):
    """env_kwargs -> config, for the device-resident envs: the integer keys the caller lists and max_distance, each only where
    `kw` has it (absent: the env's default stays)"""
    for name in int_keys:
        if name in kw:
            setattr(cfg, name, int(kw[name]))
    if "max_distance" in kw:
        cfg.max_distance = float(kw["max_distance"])


@contextlib.contextmanager
def _rollout_frame(env):
    """The frame of an enqueue-only rollout on `env` (its h, device, torch_stream): the body runs with the env's stream current,
    so the planes it allocates live (and are later freed) on the stream that fills them.  A caller on that stream is not
    synchronised at all; one on another stream is, before the body and after it."""
    ordered = torch.cuda.current_stream(env.device).cuda_stream == env.torch_stream.cuda_stream
    if not ordered:
        torch.cuda.current_stream(env.device).synchronize()
    with torch.cuda.stream(env.torch_stream):
        yield
    if not ordered:
        env.h.sync()


def _rollout_planes(env, T, obs_dim=None):
    """the new [T][N]... planes a rollout returns: "reward", "done", "actions" and, with obs_dim, "obs" in front of them"""
    n, dev = env.num_envs, env.device
    out = {} if obs_dim is None else {"obs": torch.empty((T, n, obs_dim), dtype=torch.float32, device=dev)}
    out["reward"] = torch.empty((T, n), dtype=torch.float32, device=dev)
    out["done"] = torch.empty((T, n), dtype=torch.uint8, device=dev)
    out["actions"] = (torch.empty((T, n), dtype=torch.int32, device=dev) if env.cfg.is_discrete
                      else torch.empty((T, n, env.h.action_dim), dtype=torch.float32, device=dev))
    return out


def first_done_masks(done):
    """[T][N] done plane -> bool planes (seen, before): the env has reported done at this row or an earlier one / at an EARLIER row
    (`~before`: the rows up to and including its first done — from the next one on a freeze_after_done env acts `None`)"""
    d = (done & 1) != 0                                                            # (bit 1: srlhip_config.info_bits)
    seen = torch.cumsum(d.to(torch.int32), 0) > 0
    return seen, torch.cat([torch.zeros_like(seen[:1]), seen[:-1]], 0)


class DeviceVecEnv(object):
    def __init__(self, env_id, num_envs, seed=0, env_kwargs=None, device_id=0, first_env_id=0, rng_mode=None):
        kw = dict(env_kwargs or {})
        rng_mode = rng_mode or default_rng_mode("device")
        cfg = _lib.default_config(ENV_CLASSES[env_id].ENV_KIND)
        cfg.num_envs, cfg.device_id, cfg.first_env_id, cfg.seed0 = int(num_envs), device_id, first_env_id, int(seed)
        _apply_env_kwargs(cfg, kw, ("is_discrete", "random_target", "shape_reward", "force_down", "action_repeat", "action_joints"))
        srl_model = kw.get("srl_model", "ground_truth")
        if srl_model not in OBS_MODES or srl_model == "raw_pixels":
            raise NotImplementedError("DeviceVecEnv serves the state observations; use PixelStateVecEnv for raw_pixels")
        cfg.obs_mode = OBS_MODES[srl_model]
        cfg.rng_mode, cfg.auto_reset, cfg.io_device = RNG_MODES[rng_mode], 1, 1
        self.cfg, self.env_id, self.num_envs = cfg, env_id, int(num_envs)
        self.h = _lib.Handle(cfg)
        self.device = torch.device("cuda", device_id)
        self.torch_stream = torch.cuda.ExternalStream(self.h.stream(), device=self.device)
        n = self.num_envs
        self.obs = torch.zeros((n, self.h.obs_dim), dtype=torch.float32, device=self.device)
        self.rewards = torch.zeros((n,), dtype=torch.float32, device=self.device)
        self.dones = torch.zeros((n,), dtype=torch.uint8, device=self.device)
        if cfg.is_discrete:
            self.action_space = Discrete(self.h.num_actions)
        else:
            self.action_space = Box(low=-1, high=1, shape=(self.h.action_dim,), dtype=np.float32)
        self.observation_space = Box(low=-np.inf, high=np.inf, shape=(self.h.obs_dim,), dtype=np.float32)

    def _on_env_stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream == self.torch_stream.cuda_stream

    def reset(self):
        ordered = self._on_env_stream()
        if not ordered:
            torch.cuda.current_stream(self.device).synchronize()
        self.h.reset(obs_out=self.obs.data_ptr())
        if not ordered:
            self.h.sync()
        return self.obs

    def step(self, actions):
        """actions: int32 tensor [N] (-1 == the reference's None) or float32 tensor [N, action_dim], on this device; on a Kuka env a
        continuous row of NaNs is the reference's None (include/srlhip.h: the kernels test component 0; device buffers are not checked).
        Returns (obs, rewards, dones): tensors owned by the env, overwritten by the next call."""
        want = torch.int32 if self.cfg.is_discrete else torch.float32
        assert actions.is_cuda and actions.dtype == want and actions.is_contiguous(), (actions.dtype, actions.device)
        ordered = self._on_env_stream()
        if not ordered:
            torch.cuda.current_stream(self.device).synchronize()
        self.h.step(actions.data_ptr(), out=(self.obs.data_ptr(), self.rewards.data_ptr(), self.dones.data_ptr()))
        if not ordered:
            self.h.sync()
        return self.obs, self.rewards, self.dones

    def _rollout_policy(self, call, T, params, dtype, shape, per_env, freeze_after_done, obs_mean, obs_std, clip_obs):
        """`call` (a bound Handle.rollout_policy / rollout_mlp_policy, less its leading T and parameter pointer) on tensors: `params`
        of `dtype` and `shape`, new output planes allocated on the env's stream, enqueue-only when the caller is on that stream"""
        assert params.is_cuda and params.dtype == dtype and params.is_contiguous(), (params.dtype, params.device)
        assert tuple(params.shape) == shape, (tuple(params.shape), shape)
        assert (obs_mean is None) == (obs_std is None), "obs_mean and obs_std come together"
        for x in (obs_mean, obs_std):
            assert x is None or (x.is_cuda and x.dtype == torch.float64 and x.is_contiguous() and tuple(x.shape) == (self.h.obs_dim,))
        with _rollout_frame(self):
            out = _rollout_planes(self, T, self.h.obs_dim)
            call(T, params.data_ptr(), per_env=per_env, freeze_after_done=freeze_after_done,
                 obs_mean=None if obs_mean is None else obs_mean.data_ptr(), obs_std=None if obs_std is None else obs_std.data_ptr(),
                 clip_obs=clip_obs, out=tuple(out[k].data_ptr() for k in ("obs", "reward", "done", "actions")))
        return out

    def rollout_policy(self, T, weights, per_env=True, freeze_after_done=False, obs_mean=None, obs_std=None, clip_obs=10.0, sample=False):
        """srlhip_rollout_policy on tensors: T fused steps whose actions the linear policy `weights` (float64 tensor
        [N][obs_dim][A], or [obs_dim][A] with per_env=False) picks inside the kernel from each env's own current observation.
        obs_mean / obs_std: float64 tensors [obs_dim], frozen for the call.  Enqueue-only on the env's stream (like step());
        returns {"obs", "reward", "done", "actions"}: new [T][N]... tensors of the RAW observations, rewards, dones and the
        actions taken.  The env's own obs / rewards / dones tensors are left as they were.  sample=True (discrete actions):
        srlhip_rollout_policy_sampled, the action drawn from the softmax of the scores with each env's own action stream."""
        return self._rollout_policy(functools.partial(self.h.rollout_policy, sample=True) if sample else self.h.rollout_policy, T, weights, torch.float64, self.h.policy_shape(per_env),
                                    per_env, freeze_after_done, obs_mean, obs_std, clip_obs)

    def rollout_mlp_policy(self, T, params, hidden, per_env=True, freeze_after_done=False, obs_mean=None, obs_std=None, clip_obs=10.0,
                           sample=False):
        """srlhip_rollout_mlp_policy on tensors: rollout_policy with a one-hidden-layer ReLU MLP.  `params`: float32 CUDA tensor
        [N][P] (or [P] with per_env=False), P = h.mlp_param_count(hidden), nn.Module.parameters() order.  Enqueue-only; returns
        the same dict of new [T][N]... tensors.  sample=True (discrete actions): srlhip_rollout_mlp_policy_sampled, the action drawn
        from the softmax of the scores with each env's own action stream."""
        shape = ((self.num_envs,) if per_env else ()) + (self.h.mlp_param_count(int(hidden)),)
        return self._rollout_policy(functools.partial(self.h.rollout_mlp_policy, hidden=hidden, sample=sample), T, params, torch.float32, shape,
                                    per_env, freeze_after_done, obs_mean, obs_std, clip_obs)

    def _rollout_summary(self, T, block, dtype, shape, per_env, freeze_after_done, obs_mean, obs_std, clip_obs, moments, **which):
        """Handle.rollout_policy_summary on tensors (`block`: the parameter tensor; `which`: its pointer as weights= / params= and
        hidden=, and sample=), as _rollout_policy: the four small result tensors are allocated on the env's stream, the call only
        enqueues when the caller is on that stream"""
        assert block.is_cuda and block.dtype == dtype and block.is_contiguous(), (block.dtype, block.device)
        assert tuple(block.shape) == shape, (tuple(block.shape), shape)
        assert (obs_mean is None) == (obs_std is None), "obs_mean and obs_std come together"
        for x in (obs_mean, obs_std):
            assert x is None or (x.is_cuda and x.dtype == torch.float64 and x.is_contiguous() and tuple(x.shape) == (self.h.obs_dim,))
        n, D, dev = self.num_envs, self.h.obs_dim, self.device
        with _rollout_frame(self):
            out = {"ret": torch.empty((n,), dtype=torch.float64, device=dev), "length": torch.empty((n,), dtype=torch.int32, device=dev)}
            if moments:
                out["obs_sum"] = torch.empty((n, D), dtype=torch.float64, device=dev)
                out["obs_sqsum"] = torch.empty((n, D), dtype=torch.float64, device=dev)
            self.h.rollout_policy_summary(T, per_env=per_env, freeze_after_done=freeze_after_done, moments=moments,
                                          obs_mean=None if obs_mean is None else obs_mean.data_ptr(), obs_std=None if obs_std is None else obs_std.data_ptr(),
                                          clip_obs=clip_obs, out=tuple(out[k].data_ptr() if k in out else None for k in ("ret", "length", "obs_sum", "obs_sqsum")),
                                          **which)
        return out

    def rollout_policy_summary(self, T, weights, per_env=True, freeze_after_done=False, obs_mean=None, obs_std=None, clip_obs=10.0, sample=False,
                               moments=True):
        """srlhip_rollout_policy_summary with a linear policy: rollout_policy's T fused steps (same arguments, same env state
        afterwards), returning what a learner keeps instead of the planes — {"ret" [N] float64: the rewards before each env's first
        done of the call, "length" [N] int32: its live steps, "obs_sum", "obs_sqsum" [N][obs_dim] float64 (with `moments`): the sums
        of its live raw observations and of their squares}, new tensors.  Enqueue-only on the env's stream; per-call scope (a call
        does not continue the sums of the one before it)."""
        return self._rollout_summary(T, weights, torch.float64, self.h.policy_shape(per_env), per_env, freeze_after_done, obs_mean, obs_std, clip_obs, moments,
                                     weights=weights.data_ptr(), sample=sample)

    def rollout_mlp_policy_summary(self, T, params, hidden, per_env=True, freeze_after_done=False, obs_mean=None, obs_std=None, clip_obs=10.0,
                                   sample=False, moments=True):
        """rollout_policy_summary with rollout_mlp_policy's one-hidden-layer ReLU MLP (`params`, `hidden`: as there)."""
        shape = ((self.num_envs,) if per_env else ()) + (self.h.mlp_param_count(int(hidden)),)
        return self._rollout_summary(T, params, torch.float32, shape, per_env, freeze_after_done, obs_mean, obs_std, clip_obs, moments,
                                     params=params.data_ptr(), hidden=hidden, sample=sample)

    def episode_stats(self):
        return self.h.episode_stats()

    def close(self):
        self.h.close()


class DeviceVecEnvWrapper(object):
    def __init__(self, venv, observation_space=None):
        self.venv, self.num_envs = venv, venv.num_envs
        self.observation_space = observation_space or venv.observation_space
        self.action_space = venv.action_space

    def __getattr__(self, name):
        return getattr(self.venv, name)

    def close(self):
        return self.venv.close()


class DeviceVecFrameStack(DeviceVecEnvWrapper):
    """stable_baselines.common.vec_env.VecFrameStack on tensors: newest frame last, a finished env's stack is cleared."""

    def __init__(self, venv, n_stack):
        wos = venv.observation_space
        low, high = np.repeat(wos.low, n_stack, axis=-1), np.repeat(wos.high, n_stack, axis=-1)
        super(DeviceVecFrameStack, self).__init__(venv, Box(low=low, high=high, dtype=wos.dtype))
        self.n_stack, self.stacked = n_stack, None

    def _push(self, obs, dones=None):
        last = obs.shape[-1]
        if self.stacked is None:
            self.stacked = torch.zeros((obs.shape[0], last * self.n_stack), dtype=obs.dtype, device=obs.device)
        self.stacked = torch.roll(self.stacked, shifts=-last, dims=-1)
        if dones is not None:
            self.stacked = self.stacked * (dones == 0).to(obs.dtype).unsqueeze(-1)
        self.stacked[..., -last:] = obs
        return self.stacked

    def reset(self):
        obs = self.venv.reset()
        self.stacked = None
        return self._push(obs)

    def step(self, actions):
        obs, rew, done = self.venv.step(actions)
        return self._push(obs, done), rew, done

    def _pass_through(self, name, *args, **kw):
        """The fused policy rollouts see single frames: only the trivial stack passes through."""
        if self.n_stack > 1:
            raise NotImplementedError("{}: frame stacking (n_stack > 1) is not fused; use the per-step path".format(name))
        return getattr(self.venv, name)(*args, **kw)

    def rollout_policy(self, T, weights, **kw):
        """The fused policy rollout sees single frames: only the trivial stack passes through."""
        return self._pass_through("rollout_policy", T, weights, **kw)

    def rollout_mlp_policy(self, T, params, hidden, **kw):
        """As rollout_policy: only the trivial stack passes through."""
        return self._pass_through("rollout_mlp_policy", T, params, hidden, **kw)

    def rollout_policy_summary(self, T, weights, **kw):
        """As rollout_policy: only the trivial stack passes through."""
        return self._pass_through("rollout_policy_summary", T, weights, **kw)

    def rollout_mlp_policy_summary(self, T, params, hidden, **kw):
        """As rollout_policy: only the trivial stack passes through."""
        return self._pass_through("rollout_mlp_policy_summary", T, params, hidden, **kw)


class RunningMeanStd(object):
    """stable_baselines.common.running_mean_std.RunningMeanStd (parallel-variance batch update) on tensors"""

    def __init__(self, shape, device, epsilon=1e-4):
        self.mean = torch.zeros(shape, dtype=torch.float64, device=device)
        self.var = torch.ones(shape, dtype=torch.float64, device=device)
        self.count = epsilon

    def update(self, x):
        x = x.to(torch.float64)
        bmean, bvar, bcount = x.mean(0), x.var(0, unbiased=False), x.shape[0]
        delta, tot = bmean - self.mean, self.count + bcount
        m2 = self.var * self.count + bvar * bcount + delta * delta * (self.count * bcount / tot)
        self.mean, self.var, self.count = self.mean + delta * (bcount / tot), m2 / tot, tot

    def update_weighted(self, x, w):
        """The same update for the rows of x [..., shape] whose weight w [...] is 1 (0: the row does not count), without
        gathering them: no device-to-host read.  `count` becomes a 0-d tensor."""
        x, w = x.to(torch.float64).reshape(-1, *self.mean.shape), w.to(torch.float64).reshape(-1, *([1] * self.mean.dim()))
        bcount = torch.clamp(w.sum(), min=1.0)
        bmean = (w * x).sum(0) / bcount
        bvar = (w * (x - bmean) ** 2).sum(0) / bcount
        delta, tot = bmean - self.mean, self.count + bcount
        m2 = self.var * self.count + bvar * bcount + delta * delta * (self.count * bcount / tot)
        self.mean, self.var, self.count = self.mean + delta * (bcount / tot), m2 / tot, tot

    def update_from_sums(self, count, sum, sqsum):
        """The same update from a batch given as its row count and the sums of its rows and of their squares (0-d / [shape]
        float64 tensors): batch mean = sum / n, batch variance = sqsum / n - mean^2 (clamped at 0), then the merge above.  No
        device-to-host read; `count` becomes a 0-d tensor."""
        bcount = torch.clamp(count.to(torch.float64), min=1.0)
        bmean = sum / bcount
        bvar = torch.clamp(sqsum / bcount - bmean * bmean, min=0.0)
        delta, tot = bmean - self.mean, self.count + bcount
        m2 = self.var * self.count + bvar * bcount + delta * delta * (self.count * bcount / tot)
        self.mean, self.var, self.count = self.mean + delta * (bcount / tot), m2 / tot, tot


class DeviceVecNormalize(DeviceVecEnvWrapper):
    """stable_baselines VecNormalize: obs -> clip((obs - mean) / sqrt(var + eps)), optional return-based reward scaling."""

    def __init__(self, venv, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99,
                 epsilon=1e-8):
        super(DeviceVecNormalize, self).__init__(venv)
        dev = venv.device
        self.obs_rms = RunningMeanStd(self.observation_space.shape, dev)
        self.ret_rms = RunningMeanStd((), dev)
        self.ret = torch.zeros(self.num_envs, dtype=torch.float64, device=dev)
        self.training, self.norm_obs, self.norm_reward = training, norm_obs, norm_reward
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = clip_obs, clip_reward, gamma, epsilon
        self.old_obs = None

    # same files as stable_baselines' VecNormalize (and srlhip.vec_wrappers.VecNormalize): {path}/obs_rms.pkl, ret_rms.pkl with
    # host-side (mean, var, count) objects, so statistics move freely between the host and the device wrapper
    def save_running_average(self, path):
        import pickle
        from .vec_wrappers import _RunningMeanStd as HostRms
        for rms, name in ((self.obs_rms, "obs_rms"), (self.ret_rms, "ret_rms")):
            host = HostRms(tuple(rms.mean.shape))
            host.mean, host.var, host.count = rms.mean.cpu().numpy(), rms.var.cpu().numpy(), float(rms.count)      # (count: float or 0-d tensor)
            with open("{}/{}.pkl".format(path, name), "wb") as f:
                pickle.dump(host, f)

    def load_running_average(self, path):
        import pickle
        for rms, name in ((self.obs_rms, "obs_rms"), (self.ret_rms, "ret_rms")):
            with open("{}/{}.pkl".format(path, name), "rb") as f:
                host = pickle.load(f)
            rms.mean = torch.as_tensor(np.asarray(host.mean), dtype=torch.float64, device=rms.mean.device).reshape(rms.mean.shape)
            rms.var = torch.as_tensor(np.asarray(host.var), dtype=torch.float64, device=rms.var.device).reshape(rms.var.shape)
            rms.count = float(host.count)

    saveRunningAverage, loadRunningAverage = save_running_average, load_running_average

    def _obfilt(self, obs):
        if not self.norm_obs:
            return obs
        if self.training:
            self.obs_rms.update(obs)
        out = (obs.to(torch.float64) - self.obs_rms.mean) / torch.sqrt(self.obs_rms.var + self.epsilon)
        return torch.clamp(out, -self.clip_obs, self.clip_obs).to(torch.float32)

    def get_original_obs(self):
        return self.old_obs

    def _rollout_frozen(self, call, *args, per_env=True, freeze_after_done=False, **more):
        """`call` (the wrapped env's rollout_policy / rollout_mlp_policy) on NORMALISED observations: the current statistics
        (sqrt(var + eps) as std, clip_obs) are handed to the kernel and stay frozen for the whole call.  With training = False this
        equals the per-step path.  With training = True the statistics are then updated ONCE, from the returned raw observation
        planes — only rows up to and including each env's first done when freeze_after_done is set (all rows otherwise): a different
        schedule than step()'s update before every action.  Returns the raw planes; rewards are not normalised."""
        if not self.norm_obs:
            return call(*args, per_env=per_env, freeze_after_done=freeze_after_done, **more)
        mean = self.obs_rms.mean.reshape(-1).contiguous()
        std = torch.sqrt(self.obs_rms.var + self.epsilon).reshape(-1).contiguous()
        out = call(*args, per_env=per_env, freeze_after_done=freeze_after_done, obs_mean=mean, obs_std=std, clip_obs=self.clip_obs, **more)
        if self.training:
            obs = out["obs"]
            if freeze_after_done:
                self.obs_rms.update_weighted(obs, ~first_done_masks(out["done"])[1])  # (no gather: the call stays enqueue-only)
            else:
                self.obs_rms.update(obs.reshape(-1, obs.shape[-1]))
        return out

    def rollout_policy(self, T, weights, per_env=True, freeze_after_done=False, sample=False):
        """The wrapped env's fused policy rollout on NORMALISED observations: the current statistics are handed to the kernel and
        stay frozen for the whole call; with training = True they are updated ONCE afterwards from the returned raw observation
        planes — a different schedule than step()'s update before every action (_rollout_frozen has the details).  Returns the
        raw planes; rewards are not normalised.  `sample` passes through."""
        return self._rollout_frozen(self.venv.rollout_policy, T, weights, per_env=per_env, freeze_after_done=freeze_after_done,
                                    **({"sample": True} if sample else {}))

    def rollout_mlp_policy(self, T, params, hidden, per_env=True, freeze_after_done=False, sample=False):
        """rollout_policy's schedule for the MLP policy: the current statistics are frozen for the call and, with training = True,
        updated once afterwards from the live rows of the returned raw observation planes.  `sample` passes through."""
        return self._rollout_frozen(self.venv.rollout_mlp_policy, T, params, hidden, per_env=per_env, freeze_after_done=freeze_after_done,
                                    **({"sample": True} if sample else {}))

    def _summary_frozen(self, call, *args, **more):
        """`call` (the wrapped env's rollout_policy_summary / rollout_mlp_policy_summary) as _rollout_frozen: the current statistics
        go to the kernel, frozen for the call; with training = True they are updated ONCE afterwards from the summary's sums of the
        LIVE rows (up to and including each env's first done: _rollout_frozen's update with freeze_after_done), added over the envs
        on the device — no host read.  Returns the summary; its moments are of the RAW observations.
        Two differences from the planes methods, both because the kernel sums live rows only: with training = True and
        freeze_after_done = False, _rollout_frozen updates from ALL T rows of every env, this method still from the live rows alone;
        and with training = True the moments are always computed and returned, whatever `moments` says (the update needs them)."""
        if not self.norm_obs:
            return call(*args, **more)
        mean = self.obs_rms.mean.reshape(-1).contiguous()
        std = torch.sqrt(self.obs_rms.var + self.epsilon).reshape(-1).contiguous()
        out = call(*args, obs_mean=mean, obs_std=std, clip_obs=self.clip_obs, **dict(more, moments=True if self.training else more.get("moments", True)))
        if self.training:
            shape = self.obs_rms.mean.shape
            self.obs_rms.update_from_sums(out["length"].sum(), out["obs_sum"].sum(0).reshape(shape), out["obs_sqsum"].sum(0).reshape(shape))
        return out

    def rollout_policy_summary(self, T, weights, per_env=True, freeze_after_done=False, sample=False, moments=True):
        """The wrapped env's rollout_policy_summary on NORMALISED observations: the current statistics are frozen for the call and,
        with training = True, updated ONCE afterwards from the sums of the live rows (up to and including each env's first done).
        That is rollout_policy's update with freeze_after_done = True; WITHOUT freeze_after_done rollout_policy updates from all T
        rows and this method does not (the kernel sums live rows only).  With training = True the returned dict holds "obs_sum" and
        "obs_sqsum" even with moments=False: the update needs them."""
        return self._summary_frozen(self.venv.rollout_policy_summary, T, weights, per_env=per_env, freeze_after_done=freeze_after_done, sample=sample,
                                    moments=moments)

    def rollout_mlp_policy_summary(self, T, params, hidden, per_env=True, freeze_after_done=False, sample=False, moments=True):
        """rollout_policy_summary's schedule for the MLP policy: statistics frozen for the call; with training = True one update
        afterwards from the live rows' sums — rollout_mlp_policy's update with freeze_after_done = True, NOT its all-rows update
        without it — and the moments are then returned even with moments=False."""
        return self._summary_frozen(self.venv.rollout_mlp_policy_summary, T, params, hidden, per_env=per_env, freeze_after_done=freeze_after_done,
                                    sample=sample, moments=moments)

    def reset(self):
        obs = self.venv.reset()
        self.old_obs = obs
        self.ret.zero_()
        return self._obfilt(obs)

    def step(self, actions):
        obs, rew, done = self.venv.step(actions)
        self.old_obs = obs
        self.ret = self.ret * self.gamma + rew.to(torch.float64)
        out = self._obfilt(obs)
        if self.norm_reward:
            if self.training:
                self.ret_rms.update(self.ret)
            rew = torch.clamp(rew.to(torch.float64) / torch.sqrt(self.ret_rms.var + self.epsilon), -self.clip_reward,
                              self.clip_reward).to(torch.float32)
        self.ret = self.ret * (done == 0).to(torch.float64)
        return out, rew, done
