"""rl_baselines/evolution_strategies/ars.py — Augmented Random Search (arXiv 1803.07055) with the reference's
surface (ARSModel: customArguments / getAction / getActionProba / makeEnv / train / save / load, same hyper-parameters
and update rule, ars.py:17-220), evaluated on the GPU.

The reference evaluates the 2 x n_population perturbed linear policies with a Python loop over envs around a
SubprocVecEnv step (ars.py:152-186).  Here the population is the batch: env 2k runs M + noise * delta_k, env 2k+1 runs
M - noise * delta_k; one batched matmul + argmax (or softmax sampling) produces all actions as an int32 tensor that the
stepper reads in place (DeviceVecEnv, io_device = 1), on the stepper's own HIP stream — no host round trip per step.
Finished directions receive the `None` action exactly like the reference ("do nothing, as we are done"): -1 with discrete actions,
a row of NaNs with continuous actions on the Kuka envs (include/srlhip.h), whose step then draws no noise.  MobileRobot envs with
continuous actions get zero rows instead: the reference's MobileRobotGymEnv.step has no continuous `None` (action[0] raises).

--fused-rollout (off by default; the MobileRobot envs, KukaButton / KukaMovingButton / Kuka2Button; ground-truth observations,
--deterministic or --continuous-actions, no frame stacking): one evaluation is reset + ONE srlhip_rollout_policy launch — the kernel applies each env's own M +- noise * delta to the
observation it has just produced — and the returns come from the reward / done planes.  Softmax sampling (no --deterministic)
stays on the per-step path above unless --fused-sampling is given.  (CMA-ES, whose policy is a 100-unit MLP, has its own fused form: cma_es.py.)

--fused-sampling (off by default; needs --fused-rollout and discrete actions; checked by ARSModel.check_arguments, which train() calls —
check_fused_arguments, shared with CMA-ES, keeps its verdicts): the reference's default form — no --deterministic, each
direction's action drawn from the softmax of its scores (ars.py:87-91) — in the same one launch (srlhip_rollout_policy_sampled); on a
learned SRL model and with --pixel-policy the loop of launches gains one srlhip_sample_actions per step and still has no host read.  The
action draws then come from each env's own counter-based action stream (Philox stream 1, keyed by seed and env id), not from the
`torch.multinomial` generator of the per-step path: the two paths sample the same distribution but not the same bits.  (The reference
draws from the global np.random: no per-env stream could reproduce it either.)

A learned SRL model (--srl-model autoencoder, robotic_priors, ...: state_representation/registry.py, SRLType.SRL) runs on both paths:
makeEnv then builds a PixelStateVecEnv (stepper, rasteriser, encoder on one stream) and the observation is the encoder's state vector.
--fused-returns (off by default; needs --fused-rollout on the env's own ground-truth observations): the launch returns each
direction's return and live-step count itself (srlhip_rollout_policy_summary) instead of the [T][N] planes the returns were then
reduced from — the same steps, the same returns bit for bit, no planes allocated.  With v2's normalisation the statistics are updated
from the launch's sums of the live observations (sum / n, sqsum / n - mean^2) where the planes path takes the two-pass variance: equal
up to float64 rounding.  Refused by check_returns_arguments (CMA-ES's too) where no fused kernel stands behind the rollout: learned SRL
models, --pixel-policy, --cnn-policy.

With --fused-rollout an evaluation is T x (srlhip_policy_act, step + rasteriser, encoder) enqueued by env.rollout_policy — the same
action selection as a kernel of its own, no host read in the loop.

--pixel-policy (off by default; with --srl-model raw_pixels, --num-stack 1): the reference's ARS on raw pixels — np.dot(obs.reshape(-1),
M +- noise * delta_k) on the uint8 frame as it lies, no / 255 and no VecNormalize (ars.py:85,120,162-166).  makeEnv builds a RawPixelVecEnv
and every env step is ONE srlhip_pixel_policy_act launch on the frames where the rasteriser left them: delta_k is read once for envs 2k
and 2k + 1, M stays in cache, no per-env weight block is formed.  With --deterministic or --continuous-actions the launch writes the
actions; otherwise it leaves the scores and the action is drawn from their softmax as on the state path.  --fused-rollout enqueues the
whole evaluation, T x (srlhip_pixel_policy_act, step + rasteriser), with no host read in between (env.rollout_pixel_policy); with
--fused-sampling each step also has its srlhip_sample_actions launch.  Without the flag raw_pixels is refused as before."""
import argparse
import pickle
import time

import numpy as np
import torch

from srlhip import _lib
from srlhip.device_env import DeviceVecEnv, DeviceVecFrameStack, DeviceVecNormalize, first_done_masks
from srlhip.envs import ENV_CLASSES


class ARSModel(object):
    def __init__(self):
        self.n_population = None
        self.top_population = None
        self.step_size = None
        self.exploration_noise = None
        self.continuous_actions = None
        self.max_step_amplitude = None
        self.deterministic = None
        self.M = None                     # the linear policy (numpy, like the reference: pickled by save())

    def save(self, save_path, _locals=None):
        assert self.M is not None, "Error: must train or load model before use"
        with open(save_path, "wb") as f:
            pickle.dump(self.__dict__, f)

    @classmethod
    def load(cls, load_path, args=None):
        with open(load_path, "rb") as f:
            class_dict = pickle.load(f)
        loaded_model = ARSModel()
        loaded_model.__dict__ = class_dict
        return loaded_model

    def customArguments(self, parser):
        parser.add_argument('--num-population', help='Number of population (each one has 2 envs)', type=int, default=10)
        parser.add_argument('--exploration-noise', help='The standard deviation of the exploration noise', type=float,
                            default=0.02)
        parser.add_argument('--step-size', help='The step size for param update', type=float, default=0.02)
        parser.add_argument('--top-population', help='Number of top population to use in update', type=int, default=2)
        parser.add_argument('--algo-type', help='"v1" is standard ARS, "v2" is for rolling average normalization.',
                            type=str, default="v2", choices=["v1", "v2"])
        parser.add_argument('--max-step-amplitude', type=float, default=10,
                            help='Set the maximum update vectors amplitude (mesured in factors of step_size)')
        parser.add_argument('--deterministic', action='store_true', default=False,
                            help='do a deterministic approach for the actions on the output of the policy')
        parser.add_argument('--fused-rollout', action='store_true', default=False,
                            help='evaluate each population with one fused policy rollout launch (ground-truth observations or a learned SRL model; needs '
                                 '--deterministic or --continuous-actions and --num-stack 1; not KukaRandButton). The training '
                                 'callback then fires once per evaluation, not once per env step')
        # with --fused-rollout and discrete actions: draw each action from the softmax of the scores inside the fused launch (no
        # --deterministic needed); the draws come from each env's own action stream, not from the torch.multinomial generator of the
        # per-step path: same distribution, other bits.  Documented in the module docstring and kept out of the generated help:
        # tests/test_mlp_sample_cpu.py pins this parser's help text to the one without it.
        parser.add_argument('--fused-sampling', action='store_true', default=False, help=argparse.SUPPRESS)
        parser.add_argument('--fused-returns', action='store_true', default=False,
                            help='with --fused-rollout on ground-truth observations: the launch returns each direction\'s return and live steps '
                                 'itself instead of the reward / done planes (same returns; not with a learned SRL model or --pixel-policy)')
        parser.add_argument('--pixel-policy', action='store_true', default=False,
                            help='with --srl-model raw_pixels: the linear policy on the flattened uint8 frame, run on the device from the '
                                 'rendered frames (srlhip_pixel_policy_act; --num-stack 1)')
        return parser

    # steps after which every env has reported done (`done = counter > max_steps`): MobileRobot 250 (mobile_robot_env.py:336-343),
    # KukaButton 1000, KukaMovingButton / Kuka2Button 1500
    FUSED_EPISODE_LIMIT = {_lib.ENV_MOBILE: 251, _lib.ENV_MOBILE_1D: 251, _lib.ENV_MOBILE_2TARGET: 251, _lib.ENV_MOBILE_LINE: 251,
                           _lib.ENV_KUKA_BUTTON: 1001, _lib.ENV_KUKA_MOVING: 1501, _lib.ENV_KUKA_2BUTTON: 1501}

    @staticmethod
    def check_fused_arguments(args):
        """--fused-rollout against the rest of the arguments; raises ValueError before any env is built.  (CMAESModel's too.)"""
        if not getattr(args, "fused_rollout", False):
            return
        if not (getattr(args, "deterministic", False) or getattr(args, "continuous_actions", False)):
            raise ValueError("--fused-rollout needs --deterministic or --continuous-actions: softmax sampling of the action is "
                             "not fused (it stays on the per-step path)")
        if int(getattr(args, "num_stack", 1)) != 1:
            raise ValueError("--fused-rollout needs --num-stack 1: frame stacking is not fused")
        if ARSModel.linear_from_pixels(args):
            pass                                                  # the frame itself is the observation (srlhip_pixel_policy_act)
        elif getattr(args, "srl_model", "ground_truth") != "ground_truth" and not ARSModel.learned_srl(args):
            raise ValueError("--fused-rollout needs --srl-model ground_truth or a learned SRL model (raw_pixels, joints and "
                             "joints_position are not fused)")
        if ENV_CLASSES[args.env].ENV_KIND not in ARSModel.FUSED_EPISODE_LIMIT:
            raise ValueError("--fused-rollout: {} has no fused policy rollout".format(args.env))

    @staticmethod
    def check_returns_arguments(args):
        """--fused-returns against the rest of the arguments (check_fused_arguments' sibling; CMAESModel's too): it needs
        --fused-rollout and a rollout that IS one kernel — with a learned SRL model, --pixel-policy or --cnn-policy the rollout is a
        sequence of launches per step and there is nothing to return the sums from.  Raises ValueError before any env is built."""
        if not getattr(args, "fused_returns", False):
            return
        if not getattr(args, "fused_rollout", False):
            raise ValueError("--fused-returns needs --fused-rollout")
        if getattr(args, "pixel_policy", False) or getattr(args, "cnn_policy", False):
            raise ValueError("--fused-returns: --pixel-policy / --cnn-policy rollouts are per-step launch sequences, not one fused kernel")
        if getattr(args, "srl_model", "ground_truth") != "ground_truth":
            raise ValueError("--fused-returns needs --srl-model ground_truth: a rollout on a learned SRL model is a per-step launch "
                             "sequence, not one fused kernel")

    @staticmethod
    def check_arguments(args):
        """What train() checks: --fused-returns first (check_returns_arguments), then --fused-sampling against the rest of the
        arguments (CMAESModel's rules and wording), then check_fused_arguments, whose "--deterministic or --continuous-actions"
        requirement --fused-sampling meets; raises ValueError before any env is built.  A namespace without fused_sampling:
        check_returns_arguments and check_fused_arguments alone."""
        ARSModel.check_returns_arguments(args)
        if not getattr(args, "fused_sampling", False):
            return ARSModel.check_fused_arguments(args)
        if not getattr(args, "fused_rollout", False):
            raise ValueError("--fused-sampling needs --fused-rollout")
        if getattr(args, "continuous_actions", False):
            raise ValueError("--fused-sampling needs discrete actions (not --continuous-actions): continuous actions are never sampled")
        met = type(args)(**dict(vars(args), deterministic=True))       # the other rules with that one requirement met
        return ARSModel.check_fused_arguments(met)

    @staticmethod
    def linear_from_pixels(args):
        return bool(getattr(args, "pixel_policy", False)) and getattr(args, "srl_model", "ground_truth") == "raw_pixels"

    @staticmethod
    def learned_srl(args_or_name):
        """the srl_model is a learned encoder on raw pixels (state_representation/registry.py: SRLType.SRL)"""
        from state_representation.registry import registered_srl, SRLType
        name = args_or_name if isinstance(args_or_name, str) else getattr(args_or_name, "srl_model", "ground_truth")
        return registered_srl.get(name, (None,))[0] is SRLType.SRL

    @staticmethod
    def make_base_env(args, env_kwargs):
        """The env under the wrappers: DeviceVecEnv for the env's own state observations; for a learned SRL model a
        PixelStateVecEnv — stepper, rasteriser and encoder on one stream — with the encoder resolved as HipVecEnv does
        (srl_model_path / state_dim / random-init) and the frame size from env_kwargs["img_shape"] or args.img_shape."""
        device_id = getattr(args, "device_id", 0)
        if env_kwargs["srl_model"] == "raw_pixels" and getattr(args, "pixel_policy", False):
            if int(getattr(args, "num_stack", 1)) != 1:
                raise ValueError("--pixel-policy needs --num-stack 1: the policy reads one frame")
            from srlhip.pixel_env import RawPixelVecEnv
            from srlhip.vec_env import RNG_MODES, default_rng_mode
            img_shape = tuple(env_kwargs.get("img_shape") or getattr(args, "img_shape", None) or (224, 224))[-2:]
            return RawPixelVecEnv(args.env, args.num_cpu, seed=args.seed, img_shape=img_shape, device_id=device_id,
                                  rng_mode=RNG_MODES[default_rng_mode("device")], env_kwargs=env_kwargs)
        if not ARSModel.learned_srl(env_kwargs["srl_model"]):
            return DeviceVecEnv(args.env, args.num_cpu, seed=args.seed, env_kwargs=env_kwargs, device_id=device_id)
        from srlhip.pixel_env import PixelStateVecEnv
        from srlhip.vec_env import RNG_MODES, default_rng_mode, resolve_encoder
        kw = dict(env_kwargs)
        for name in ("srl_model_path", "state_dim"):
            if name not in kw and getattr(args, name, None) is not None:
                kw[name] = getattr(args, name)
        img_shape = tuple(kw.get("img_shape") or getattr(args, "img_shape", None) or (224, 224))[-2:]
        n_channels = 6 if (kw.get("multi_view") or kw.get("fpv")) else 3
        encoder = resolve_encoder(kw, img_shape, n_channels, torch.device("cuda", device_id))
        return PixelStateVecEnv(args.env, args.num_cpu, encoder, seed=args.seed, img_shape=img_shape, device_id=device_id,
                                rng_mode=RNG_MODES[default_rng_mode("device")], env_kwargs=kw)

    @staticmethod
    def returns_from_planes(reward, done):
        """The reference's return rule (ars.py:178-180) on [T][N] reward / done planes: a step's reward counts only while the env
        has not reported done, the reporting step included -> (float64 returns [N], number of rows in which some env was still live
        when it acted)."""
        seen, before = first_done_masks(done)
        ret = (reward.to(torch.float64) * (~seen).to(torch.float64)).sum(0)
        return ret, (~before).any(dim=1).sum()

    def evaluate_fused(self, env, M, delta, T):
        """One evaluation of the population in one launch (the env was just reset): env 2k runs M + noise * delta_k, env 2k + 1
        runs M - noise * delta_k, frozen after its first done -> (returns [P][2] float64, rows in which some direction was live).
        A model that is neither deterministic nor continuous samples its actions (the argument rules have asked for --fused-sampling)."""
        P, (D, A) = delta.shape[0], M.shape
        sample = self.deterministic is False and not self.continuous_actions       # (None, a model train() has not configured: the argmax)
        kw = {"sample": True} if sample else {}
        if hasattr(env, "rollout_pixel_policy"):           # --pixel-policy: M and delta as they are, no W
            planes = env.rollout_pixel_policy(T, M, delta, self.exploration_noise, freeze_after_done=True, **kw)
            ret, live_rows = self.returns_from_planes(planes["reward"], planes["done"])
            return ret.view(P, 2), int(live_rows)
        sign = torch.tensor([1.0, -1.0], dtype=M.dtype, device=M.device).view(1, 2, 1, 1)
        W = (M.unsqueeze(0).unsqueeze(0) + self.exploration_noise * sign * delta.unsqueeze(1)).reshape(2 * P, D, A).contiguous()
        if getattr(self, "fused_returns", False):          # --fused-returns: the launch reduces; moments only where a wrapper wants them
            out = env.rollout_policy_summary(T, W, per_env=True, freeze_after_done=True, moments=False, **kw)
            return out["ret"].view(P, 2), int(out["length"].max())
        planes = env.rollout_policy(T, W, per_env=True, freeze_after_done=True, **kw)
        ret, live_rows = self.returns_from_planes(planes["reward"], planes["done"])
        return ret.view(P, 2), int(live_rows)

    @classmethod
    def getOptParam(cls):
        return {"top_population": (int, (1, 5)), "exploration_noise": (float, (0, 0.1)), "step_size": (float, (0, 0.1)),
                "max_step_amplitude": (float, (1, 100))}

    # ---- host-side single-policy interface (replay / enjoy: rl_baselines/evolution_strategies/ars.py:77-104) ------
    def _scores(self, observation, delta=0):
        assert self.M is not None, "Error: must train or load model before use"
        obs = np.asarray(observation, dtype=np.float64)
        if obs.ndim > 2:                                   # image observations [n][H][W][C]: the flattened frame, as it lies
            obs = obs.reshape(len(obs), -1)
        return np.atleast_2d(obs) @ (self.M + delta)

    def getActionProba(self, observation, dones=None, delta=0):
        """Continuous actions: the linear policy's output; discrete: its softmax, one row per observation."""
        scores = self._scores(observation, delta)
        if self.continuous_actions:
            return scores
        z = np.exp(scores - scores.max(axis=1, keepdims=True))
        return z / z.sum(axis=1, keepdims=True)

    def getAction(self, observation, dones=None, delta=0):
        if self.continuous_actions:
            return self._scores(observation, delta)
        if self.deterministic:
            return self._scores(observation, delta).argmax(axis=1)
        cdf = np.cumsum(self.getActionProba(observation, delta=delta), axis=1)          # inverse-CDF sampling, all rows at once
        return (np.random.random_sample((len(cdf), 1)) * cdf[:, -1:] < cdf).argmax(axis=1)

    # ---- env assembly: ars.py:107-126 with the device-resident stack ----------------------------------------------
    @classmethod
    def makeEnv(cls, args, env_kwargs=None, load_path_normalise=None):
        if "num_population" in args.__dict__:
            args.num_cpu = args.num_population * 2
        env_kwargs = dict(env_kwargs or {})
        env_kwargs.setdefault("srl_model", getattr(args, "srl_model", "ground_truth"))
        envs = cls.make_base_env(args, env_kwargs)
        if cls.linear_from_pixels(args):
            return envs                                    # the frames themselves: no stack, no VecNormalize (ars.py:120)
        envs = DeviceVecFrameStack(envs, getattr(args, "num_stack", 1))
        if getattr(args, "srl_model", "ground_truth") != "raw_pixels" and getattr(args, "algo_type", "v2") == "v2":
            envs = DeviceVecNormalize(envs, norm_obs=True, norm_reward=False)
            if load_path_normalise is not None:        # replay: frozen statistics of the training run (rl_baselines/utils.py:232-237)
                envs.training = False
                envs.load_running_average(load_path_normalise)
        return envs

    @staticmethod
    def batched_actions(obs, M, delta, noise, active, continuous, deterministic, generator=None, none_rows=False):
        """obs [2P, D] (env 2k = +delta_k, env 2k+1 = -delta_k), M [D, A], delta [P, D, A] -> actions for every env.
        Discrete: int32 [2P] with -1 (the reference's `None`) for finished directions.  Continuous: float32 [2P, A]; a finished
        direction gets a row of NaNs with `none_rows` (the Kuka envs' `None`, include/srlhip.h: no noise draw, as in the reference,
        ars.py:168-172) and zeros otherwise (MobileRobot: the reference's step has no continuous `None`)."""
        P = delta.shape[0]
        sign = torch.tensor([1.0, -1.0], dtype=M.dtype, device=M.device).view(1, 2, 1, 1)
        W = M.unsqueeze(0).unsqueeze(0) + noise * sign * delta.unsqueeze(1)              # [P, 2, D, A]
        out = torch.matmul(obs.view(P, 2, 1, -1).to(M.dtype), W).view(2 * P, -1)       # [2P, A]
        if continuous:
            if none_rows:
                return torch.where(active.unsqueeze(-1), out, torch.full_like(out, float("nan"))).to(torch.float32).contiguous()
            return (out * active.unsqueeze(-1).to(out.dtype)).to(torch.float32).contiguous()
        if deterministic:
            a = torch.argmax(out, dim=1)
        else:
            a = torch.multinomial(torch.softmax(out, dim=1), 1, generator=generator).squeeze(1)
        return torch.where(active, a, torch.full_like(a, -1)).to(torch.int32).contiguous()

    @staticmethod
    def pixel_actions(env, M, delta, noise, done, frozen, scores, continuous, deterministic, generator=None):
        """batched_actions for --pixel-policy: ONE srlhip_pixel_policy_act launch on the frames the env holds.  `done` (bool [2P]) is
        copied into the call's frozen plane, so finished directions get the `None` rows batched_actions writes (-1; NaN rows on the
        Kuka envs, zero rows on MobileRobot).  Deterministic or continuous: the kernel's own selection; otherwise the scores come
        back in `scores` and the action is drawn from their softmax."""
        frozen.copy_(done)
        with torch.cuda.stream(env.torch_stream):
            h = env.h
            actions = torch.empty_like(env.actions)
            h.pixel_policy_act(env.images.data_ptr(), actions.data_ptr(), M.data_ptr(), delta=delta.data_ptr(), noise=noise,
                               freeze_after_done=True, frozen=frozen.data_ptr(), score_out=scores.data_ptr())
        if continuous or deterministic:
            return actions
        a = torch.multinomial(torch.softmax(scores, dim=1), 1, generator=generator).squeeze(1)
        return torch.where(~done, a, torch.full_like(a, -1)).to(torch.int32).contiguous()

    def train(self, args, callback=None, env_kwargs=None, train_kwargs=None):
        assert args.top_population <= args.num_population, \
            "Cannot select top %d, from population of %d." % (args.top_population, args.num_population)
        assert args.num_population > 1, "The population cannot be less than 2."
        merged = dict(vars(args), **(train_kwargs or {}))
        self.check_arguments(type(args)(**merged))                # at argument time: before any env is built
        env = self.makeEnv(args, env_kwargs)
        args.__dict__.update(train_kwargs or {})
        fused = bool(getattr(args, "fused_rollout", False))
        pixels = self.linear_from_pixels(args)
        fused_T = self.FUSED_EPISODE_LIMIT.get(ENV_CLASSES[args.env].ENV_KIND, 0) + 1
        continuous = bool(getattr(args, "continuous_actions", False))
        none_rows = continuous and ENV_CLASSES[args.env].ENV_KIND >= _lib.ENV_KUKA_BUTTON      # finished directions: `None` where the reference has it
        action_space = int(np.prod(env.action_space.shape)) if continuous else env.action_space.n
        obs_dim = int(np.prod(env.observation_space.shape))
        self.n_population, self.top_population = args.num_population, args.top_population
        self.step_size, self.exploration_noise = args.step_size, args.exploration_noise
        self.continuous_actions, self.max_step_amplitude = continuous, args.max_step_amplitude
        self.deterministic = bool(getattr(args, "deterministic", False))
        self.fused_returns = bool(getattr(args, "fused_returns", False))
        self.M = np.zeros((obs_dim, action_space))
        num_updates = int(args.num_timesteps) // args.num_population * 2
        P, dev = self.n_population, env.device
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(args.seed))
        M = torch.zeros((obs_dim, action_space), dtype=torch.float64, device=dev)
        start_time, step = time.time(), 0
        self.history = []
        log_dir = getattr(args, "log_dir", None)
        with torch.cuda.stream(env.torch_stream):          # policy math and stepper kernels on ONE stream: no host syncs
            while step < num_updates:
                delta = torch.randn((P, obs_dim, action_space), dtype=torch.float64, device=dev, generator=gen)
                step0 = step
                obs = env.reset()
                if fused:
                    r, live_rows = self.evaluate_fused(env, M, delta, fused_T)
                    step = step0 + P * live_rows
                    if callback is not None:
                        callback(locals(), globals())              # once per evaluation on this path
                else:
                    r = torch.zeros((P, 2), dtype=torch.float64, device=dev)
                    done = torch.zeros(2 * P, dtype=torch.bool, device=dev)
                    live_steps = torch.zeros((), dtype=torch.int64, device=dev)      # env steps taken while some direction was still running
                    if pixels:
                        frozen = torch.zeros(2 * P, dtype=torch.uint8, device=dev)
                        scores = torch.zeros((2 * P, action_space), dtype=torch.float64, device=dev)
                    while True:
                        if pixels:
                            actions = self.pixel_actions(env, M, delta, self.exploration_noise, done, frozen, scores, continuous,
                                                         self.deterministic, gen)
                        else:
                            actions = self.batched_actions(obs, M, delta, self.exploration_noise, ~done, continuous,
                                                           self.deterministic, gen, none_rows)
                        live_steps += (~done).any().to(torch.int64)
                        obs, reward, new_done = env.step(actions)
                        step += P
                        done = done | (new_done != 0)
                        # cumulate the reward for every direction that is not finished (ars.py:178-180: after the update of `done`)
                        r += (reward.to(torch.float64) * (~done).to(torch.float64)).view(P, 2)
                        if callback is not None:
                            callback(locals(), globals())
                        if (step // P) % 16 == 0 and bool(done.all()):      # the only device->host read: every 16 env steps
                            step = step0 + P * int(live_steps)                # the <= 15 idle steps since the last direction ended do not count
                            break
                        if (step / P + 1) % 500 == 0:
                            print("{} steps - {:.2f} FPS".format(step, step / (time.time() - start_time)))
                idx = torch.argsort(r.max(dim=1).values, descending=True)[:self.top_population]
                top = r[idx]
                delta_sum = ((top[:, 0] - top[:, 1]).view(-1, 1, 1) * delta[idx]).sum(0)
                # the normalisation of step_size guards against zero variance on sparse rewards (ars.py:196-199)
                denom = torch.clamp(self.top_population * top.std(unbiased=False), min=1.0 / self.max_step_amplitude)
                M = M + (self.step_size / denom) * delta_sum
                self.M = M.cpu().numpy()                   # callbacks may save() the model at any time
                self.history.append(float(r.mean()))
        self.M = M.cpu().numpy()
        if log_dir is not None and hasattr(env, "save_running_average"):      # the policy was trained on normalised observations
            env.save_running_average(log_dir)
        env.close()
        return self
