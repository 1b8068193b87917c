"""raw_pixels -> SRL state pipeline on one device (BASELINE configs 4-5): the stepper and the tile
rasteriser write uint8 images straight into a torch-owned HBM buffer (io_device = 1, zero host copies),
and the SRL encoder runs one batched forward on it — instead of the reference's one-image-at-a-time
encoder server behind multiprocessing queues (rl_baselines/utils.py:162-191).

rollout_policy / rollout_mlp_policy run a policy on those states without leaving the device: T x (srlhip_policy_act -> step +
rasteriser -> encoder) enqueued on the handle's stream, DeviceVecEnv's signatures and result dict, so that DeviceVecFrameStack(.., 1),
DeviceVecNormalize and the ARS / CMA-ES learners sit on this env as they do on DeviceVecEnv.  A sampled LINEAR policy (ARS's default
form; rollout_policy(sample=True), RawPixelVecEnv.rollout_pixel_policy(sample=True)) takes one launch more per step: the policy call leaves
its scores, srlhip_sample_actions draws from them with each env's own action stream — still no host read in the loop."""
import functools

import numpy as np
import torch

from . import _lib
from .device_env import _apply_env_kwargs, _rollout_frame, _rollout_planes
from .envs import ENV_CLASSES
from .gym_compat import Box, Discrete


class _PixelHandleEnv(object):
    """A raw_pixels, device-pointer handle with what every env on it holds: the frame, reward, done and action tensors the stepper
    and the rasteriser write, the action space, the handle's stream as a torch stream — and the one loop behind every policy rollout."""

    def __init__(self, env_id, num_envs, seed, img_shape, device_id, first_env_id, rng_mode, env_kwargs):
        kw = dict(env_kwargs or {})
        cfg = _lib.default_config(ENV_CLASSES[env_id].ENV_KIND)
        cfg.num_envs, cfg.device_id, cfg.first_env_id, cfg.seed0 = num_envs, device_id, first_env_id, seed
        cfg.random_target, cfg.multi_view = int(kw.get("random_target", False)), int(bool(kw.get("multi_view", False)) or bool(kw.get("fpv", False)))
        cfg.obs_mode, cfg.img_h, cfg.img_w = _lib.OBS_RAW_PIXELS, img_shape[0], img_shape[1]
        cfg.rng_mode, cfg.auto_reset, cfg.io_device = rng_mode, 1, 1
        _apply_env_kwargs(cfg, kw, ("is_discrete", "shape_reward", "force_down", "action_repeat"))
        self.h = _lib.Handle(cfg)
        self.cfg, self.env_id, self.num_envs = cfg, env_id, num_envs
        self.device = torch.device("cuda", device_id)
        ch = 6 if cfg.multi_view else 3
        self.images = torch.zeros((num_envs, img_shape[0], img_shape[1], ch), dtype=torch.uint8, device=self.device)
        self.rewards = torch.zeros((num_envs,), dtype=torch.float32, device=self.device)
        self.dones = torch.zeros((num_envs,), dtype=torch.uint8, device=self.device)
        if cfg.is_discrete:
            self.actions = torch.zeros((num_envs,), dtype=torch.int32, device=self.device)
            self.action_space = Discrete(self.h.num_actions)
        else:
            self.actions = torch.zeros((num_envs, self.h.action_dim), dtype=torch.float32, device=self.device)
            self.action_space = Box(low=-1, high=1, shape=(self.h.action_dim,), dtype=np.float32)
        self._stream_ptr = self.h.stream()
        self._stream = self.torch_stream = torch.cuda.ExternalStream(self._stream_ptr, device=self.device)

    def _rollout_loop(self, T, act, freeze_after_done, draw=False, obs_dim=None, after_step=None):
        """T x (act [-> srlhip_sample_actions] -> step + rasteriser [-> after_step]) on the handle's stream: no host read, and no
        synchronisation when the caller is on that stream.  Every kernel writes straight into row t of the new [T][N]... planes:
        `act(act_t, done_prev=, frozen=, score_out=)` (raw device pointers) launches the policy's action kernel, which reads row t - 1
        of the done plane (none at t = 0) and writes row t of the action plane; the stepper reads that row, writes row t of reward /
        done and redraws the frame buffer in place.  draw: the action kernel leaves its float64 scores and srlhip_sample_actions draws
        from them with each env's own action stream (one launch more per step); it sees the frozen plane only with
        freeze_after_done, the action kernel always.  obs_dim: the result has an "obs" plane, and after_step(obs_t) fills its row t."""
        with _rollout_frame(self):
            out = _rollout_planes(self, T, obs_dim)
            frozen = torch.zeros((self.num_envs,), dtype=torch.uint8, device=self.device)
            scores = torch.empty((self.num_envs, self.h.num_actions), dtype=torch.float64, device=self.device) if draw else None
            images = self.images.data_ptr()
            for t in range(T):
                act_t = out["actions"][t].data_ptr()
                act(act_t, done_prev=out["done"][t - 1].data_ptr() if t else None, frozen=frozen.data_ptr(),
                    score_out=scores.data_ptr() if draw else None)
                if draw:
                    self.h.sample_actions(scores.data_ptr(), act_t, frozen=frozen.data_ptr() if freeze_after_done else None)
                self.h.step(act_t, out=(images, out["reward"][t].data_ptr(), out["done"][t].data_ptr()))
                if after_step is not None:
                    after_step(out["obs"][t])
        return out

    def episode_stats(self):
        return self.h.episode_stats()


class PixelStateVecEnv(_PixelHandleEnv):
    def __init__(self, env_id, num_envs, encoder, seed=0, img_shape=(64, 64), device_id=0, first_env_id=0,
                 rng_mode=_lib.RNG_PHILOX, env_kwargs=None, use_graph=False):
        super(PixelStateVecEnv, self).__init__(env_id, num_envs, seed, img_shape, device_id, first_env_id, rng_mode, env_kwargs)
        self.encoder = encoder
        self.state_dim = int(encoder.state_dim)
        self.observation_space = Box(low=-np.inf, high=np.inf, shape=(self.state_dim,), dtype=np.float32)
        self.states = torch.zeros((num_envs, encoder.state_dim), dtype=torch.float32, device=self.device)
        self._current = None              # the float32 states the env holds now (reset / step: self.states; a rollout: its last row)
        # use_graph: replay stepper + rasteriser + encoder of a step from a HIP graph (srlhip_graph_*), keyed by the action
        # source.  Off by default: at 4096 envs the step is GPU-bound and the host already runs ahead of it (697 us eager
        # vs 702 us replayed, profiles/pixel_step_microbench.py); it pays when the host thread is the bottleneck.
        self.use_graph, self._graphs, self._warm = bool(use_graph), {}, {}

    def _encode(self):
        if self.encoder.hip is not None:
            # HIP encoder (CustomCNN kernels, or the PCA projection): enqueue on the stepper's own stream right behind the rasteriser (no host sync), then
            # order torch's current stream behind it so the caller can consume states / rewards / dones as usual
            states = self.encoder.getStates(self.images, stream=self._stream_ptr, out=self.states)
            torch.cuda.current_stream(self.device).wait_stream(self._stream)
            self._current = states
            return states
        self.h.sync()                                  # images were written on the stepper's stream
        states = self.encoder.getStates(self.images)
        self._current = states
        return states

    def reset(self):
        self._stream.wait_stream(torch.cuda.current_stream(self.device))
        self.h.reset(obs_out=self.images.data_ptr())
        return self._encode()

    def step(self, actions=None):
        """actions: int32 device tensor [N] (None -> device-sampled random agent).  -> states, rewards, dones
        (device tensors, overwritten by the next call)."""
        # the stepper's stream overwrites images / states / rewards / dones: wait for their readers (and for `actions`)
        self._stream.wait_stream(torch.cuda.current_stream(self.device))
        fused = self.encoder.hip is not None
        key = "sampled" if actions is None else ("given", actions.data_ptr())
        g = self._graphs.get(key) if (fused and self.use_graph) else None
        if g is not None:
            # stepper + rasteriser + encoder of one VecEnv step replayed from a HIP graph: one launch instead of three
            self.h.graph_launch(g)
            torch.cuda.current_stream(self.device).wait_stream(self._stream)
            self._current = self.states
            return self.states, self.rewards, self.dones
        # the first call runs eagerly (lazy allocations); at most a handful of distinct action buffers get their own graph
        capture = fused and self.use_graph and self._warm.get(key, 0) >= 1 and len(self._graphs) < 8
        if capture:
            self.h.graph_begin()
        if actions is None:
            self.h.rollout(1, out=(self.images.data_ptr(), self.rewards.data_ptr(), self.dones.data_ptr(), self.actions.data_ptr()))
        else:
            self.h.step(actions.data_ptr(), out=(self.images.data_ptr(), self.rewards.data_ptr(), self.dones.data_ptr()))
        if capture:
            self.encoder.getStates(self.images, stream=self._stream_ptr, out=self.states)
            self._graphs[key] = self.h.graph_end()
            self.h.graph_launch(self._graphs[key])                              # the captured step has not run yet
            torch.cuda.current_stream(self.device).wait_stream(self._stream)
            self._current = self.states
            return self.states, self.rewards, self.dones
        self._warm[key] = self._warm.get(key, 0) + 1
        return self._encode(), self.rewards, self.dones

    # ---- policy rollouts on the learned states: T x (srlhip_policy_act -> step + rasteriser -> encoder), enqueue-only ----------------
    def _rollout(self, T, policy, sample, per_env, freeze_after_done, obs_mean, obs_std, clip_obs):
        """`policy`: the keyword arguments of Handle.policy_act that name the policy (raw device pointers).  _rollout_loop from the
        states the env holds (after reset(), step() or an earlier rollout): the action kernel reads row t - 1 of the state plane,
        the encoder writes row t."""
        assert self._current is not None, "reset() the env first"
        D = self.state_dim
        assert (obs_mean is None) == (obs_std is None), "obs_mean and obs_std come together"
        for x in (obs_mean, obs_std):
            assert x is None or (x.is_cuda and x.dtype == torch.float64 and x.is_contiguous() and tuple(x.shape) == (D,))
        # a sampled LINEAR policy: srlhip_policy_act leaves its scores, srlhip_sample_actions draws from them
        draw = sample and "weights" in policy
        kw = dict(policy, per_env=per_env, freeze_after_done=freeze_after_done, clip_obs=clip_obs, sample=sample and not draw,
                  obs_mean=None if obs_mean is None else obs_mean.data_ptr(), obs_std=None if obs_std is None else obs_std.data_ptr())
        state = [self._current]

        def act(act_t, **planes):
            if state[0].dtype != torch.float32:            # (the first step of a torch-backend encoder: converted on the env's stream, as the planes are)
                state[0] = state[0].to(torch.float32)
            self.h.policy_act(state[0].data_ptr(), D, act_t, **planes, **kw)

        def encode(obs_t):
            if self.encoder.hip is not None:
                self.encoder.getStates(self.images, stream=self._stream_ptr, out=obs_t)
            else:                                          # no HIP backend (backend="torch", uncovered shapes): the torch forward, ordered on this stream
                obs_t.copy_(self.encoder.getStates(self.images))
            state[0] = obs_t

        out = self._rollout_loop(T, act, freeze_after_done, draw=draw, obs_dim=D, after_step=encode)
        self._current = state[0]
        return out

    def rollout_policy(self, T, weights, per_env=True, freeze_after_done=False, obs_mean=None, obs_std=None, clip_obs=10.0, sample=False):
        """DeviceVecEnv.rollout_policy on the learned states: T steps whose actions the linear policy `weights` (float64 CUDA tensor
        [N][state_dim][A], or [state_dim][A] with per_env=False) picks on the device from the state the encoder has just produced
        (srlhip_policy_act).  Returns {"obs", "reward", "done", "actions"}: new [T][N]... tensors; "obs" holds the float32 states the
        policy saw NEXT (row t: the state after step t).  The env's own states / rewards / dones tensors are left as they were.
        sample=True (discrete actions): T x (srlhip_policy_act for the scores, srlhip_sample_actions, step + rasteriser, encoder) — the
        action drawn from the softmax of the scores with each env's own action stream, still without a host read in the loop."""
        A = self.h.num_actions if self.cfg.is_discrete else self.h.action_dim
        shape = ((self.num_envs,) if per_env else ()) + (self.state_dim, A)
        assert weights.is_cuda and weights.dtype == torch.float64 and weights.is_contiguous() and tuple(weights.shape) == shape, (tuple(weights.shape), shape)
        return self._rollout(T, {"weights": weights.data_ptr()}, bool(sample), per_env, freeze_after_done, obs_mean, obs_std, clip_obs)

    def mlp_param_count(self, hidden):
        A = self.h.num_actions if self.cfg.is_discrete else self.h.action_dim
        return hidden * self.state_dim + hidden + A * hidden + A

    def rollout_mlp_policy(self, T, params, hidden, per_env=True, freeze_after_done=False, obs_mean=None, obs_std=None, clip_obs=10.0,
                           sample=False):
        """DeviceVecEnv.rollout_mlp_policy on the learned states.  `params`: float32 CUDA tensor [N][P] (or [P]), P =
        mlp_param_count(hidden) with D = state_dim; sample=True (discrete actions): the action drawn from the softmax of the scores
        with each env's own action stream, one block per env and step."""
        shape = ((self.num_envs,) if per_env else ()) + (self.mlp_param_count(int(hidden)),)
        assert params.is_cuda and params.dtype == torch.float32 and params.is_contiguous() and tuple(params.shape) == shape, (tuple(params.shape), shape)
        return self._rollout(T, {"params": params.data_ptr(), "hidden": int(hidden)}, bool(sample), per_env, freeze_after_done,
                             obs_mean, obs_std, clip_obs)

    def close(self):
        for g in self._graphs.values():
            self.h.graph_destroy(g)
        self._graphs = {}
        self.h.close()


class RawPixelVecEnv(_PixelHandleEnv):
    """The raw_pixels form without an encoder: the observation IS the uint8 frame the rasteriser writes, and the policy is the
    reference's CNN-from-pixels (CMA-ES: CNNPolicyPytorch), one network per env, run by srlhip_cnn_policy_act on the frame where it
    lies.  Constructor arguments as PixelStateVecEnv's less the encoder; reset() / step(actions) return the image tensor
    ([N][H][W][C] uint8, overwritten by the next call), rewards and dones on the device."""

    def __init__(self, env_id, num_envs, seed=0, img_shape=(64, 64), device_id=0, first_env_id=0, rng_mode=_lib.RNG_PHILOX, env_kwargs=None):
        super(RawPixelVecEnv, self).__init__(env_id, num_envs, seed, img_shape, device_id, first_env_id, rng_mode, env_kwargs)
        self.observation_space = Box(low=0, high=255, shape=tuple(self.images.shape[1:]), dtype=np.uint8)
        self._ready = False               # the frame buffer holds the env's current frame (after reset / step / a rollout)

    def cnn_param_count(self):
        return self.h.cnn_param_count()

    def reset(self):
        self._stream.wait_stream(torch.cuda.current_stream(self.device))
        self.h.reset(obs_out=self.images.data_ptr())
        torch.cuda.current_stream(self.device).wait_stream(self._stream)
        self._ready = True
        return self.images

    def step(self, actions):
        """actions: device tensor, int32 [N] or float32 [N][action_dim] -> images, rewards, dones (overwritten by the next call)"""
        self._stream.wait_stream(torch.cuda.current_stream(self.device))
        self.h.step(actions.data_ptr(), out=(self.images.data_ptr(), self.rewards.data_ptr(), self.dones.data_ptr()))
        torch.cuda.current_stream(self.device).wait_stream(self._stream)
        return self.images, self.rewards, self.dones

    def _check_params(self, params, per_env):
        shape = ((self.num_envs,) if per_env else ()) + (self.cnn_param_count(),)
        assert params.is_cuda and params.dtype == torch.float32 and params.is_contiguous() and tuple(params.shape) == shape, (tuple(params.shape), shape)

    def cnn_policy_act(self, params, per_env=True, sample=False, act_out=None, score_out=None):
        """the CNN's actions for the frames the env holds now -> the action tensor (self.actions unless act_out is given); enqueued on
        the handle's stream, the caller's stream ordered behind it"""
        assert self._ready, "reset() the env first"
        self._check_params(params, per_env)
        act = self.actions if act_out is None else act_out
        self._stream.wait_stream(torch.cuda.current_stream(self.device))
        self.h.cnn_policy_act(self.images.data_ptr(), act.data_ptr(), params.data_ptr(), per_env=per_env, sample=sample,
                              score_out=None if score_out is None else score_out.data_ptr())
        torch.cuda.current_stream(self.device).wait_stream(self._stream)
        return act

    def rollout_cnn_policy(self, T, params, per_env=True, freeze_after_done=False, sample=False):
        """T x (srlhip_cnn_policy_act, step + rasteriser) on the handle's stream, enqueue-only (_rollout_loop): the
        action kernel reads the frame buffer and row t - 1 of the done plane and writes row t of the action plane, the stepper reads
        that row, writes row t of reward / done and redraws the frames in place.  `params`: float32 CUDA tensor [N][P] (or [P]),
        P = cnn_param_count() — a CMA-ES population as it is.  Returns {"reward", "done", "actions"}: new [T][N]... tensors (no
        observation plane: T frames per env is gigabytes)."""
        assert self._ready, "reset() the env first"
        self._check_params(params, per_env)
        act = functools.partial(self.h.cnn_policy_act, self.images.data_ptr(), params=params.data_ptr(), per_env=per_env,
                                freeze_after_done=freeze_after_done, sample=sample)
        return self._rollout_loop(T, act, freeze_after_done)

    def _check_pixel_policy(self, weights, delta):
        D, A = int(np.prod(self.images.shape[1:])), self.h.num_actions if self.cfg.is_discrete else self.h.action_dim
        assert weights.is_cuda and weights.dtype == torch.float64 and weights.is_contiguous() and tuple(weights.shape) == (D, A), (tuple(weights.shape), (D, A))
        if delta is not None:
            assert self.num_envs % 2 == 0, "a paired population needs an even number of envs"
            shape = (self.num_envs // 2, D, A)
            assert delta.is_cuda and delta.dtype == torch.float64 and delta.is_contiguous() and tuple(delta.shape) == shape, (tuple(delta.shape), shape)

    def pixel_policy_act(self, weights, delta=None, noise=0.0, act_out=None, score_out=None):
        """ARS's linear policy on the frames the env holds now (srlhip_pixel_policy_act) -> the action tensor (self.actions unless
        act_out is given).  weights: float64 CUDA tensor M [D][A], D = H W C; delta: float64 [N / 2][D][A] — env 2k acts with
        M + noise delta[k], env 2k + 1 with M - noise delta[k] — or None: every env acts with M.  score_out: optional float64 [N][A]
        tensor that receives the scores.  Enqueued on the handle's stream, the caller's stream ordered behind it"""
        assert self._ready, "reset() the env first"
        self._check_pixel_policy(weights, delta)
        act = self.actions if act_out is None else act_out
        self._stream.wait_stream(torch.cuda.current_stream(self.device))
        self.h.pixel_policy_act(self.images.data_ptr(), act.data_ptr(), weights.data_ptr(), delta=None if delta is None else delta.data_ptr(),
                                noise=noise, score_out=None if score_out is None else score_out.data_ptr())
        torch.cuda.current_stream(self.device).wait_stream(self._stream)
        return act

    def rollout_pixel_policy(self, T, weights, delta=None, noise=0.0, freeze_after_done=False, sample=False):
        """T x (srlhip_pixel_policy_act, step + rasteriser) on the handle's stream, enqueue-only as rollout_cnn_policy is: an ARS
        population as it is — M, the directions delta as torch.randn((P, D, A)) left them, the exploration noise — with no per-env
        weight block formed.  Returns {"reward", "done", "actions"}: new [T][N]... tensors.  sample=True (discrete actions): T x
        (srlhip_pixel_policy_act for the scores, srlhip_sample_actions, step + rasteriser) — ARS's default form, the action drawn from the
        softmax of the scores with each env's own action stream; no host read in the loop."""
        assert self._ready, "reset() the env first"
        self._check_pixel_policy(weights, delta)
        act = functools.partial(self.h.pixel_policy_act, self.images.data_ptr(), weights=weights.data_ptr(),
                                delta=None if delta is None else delta.data_ptr(), noise=noise, freeze_after_done=freeze_after_done)
        return self._rollout_loop(T, act, freeze_after_done, draw=bool(sample))

    def close(self):
        self.h.close()
