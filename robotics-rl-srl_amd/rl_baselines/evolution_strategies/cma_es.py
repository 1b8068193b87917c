"""rl_baselines/evolution_strategies/cma_es.py — CMA-ES with the reference's surface (CMAESModel: customArguments /
getAction / getActionProba / makeEnv / train / save / load, cma_es.py:24-140), evaluated on the GPU.

The reference asks the `cma` package for `num_population` parameter vectors of a small PyTorch MLP (observation -> 100 ->
actions, cma_es.py:98-105,307-326), then loops over the population in Python — set the parameters, forward ONE observation
— around a SubprocVecEnv step, `None` for finished members (cma_es.py:114-135; here -1 with discrete actions, a row of NaNs with
continuous actions on the Kuka envs — include/srlhip.h, no noise draw — and a zero row on MobileRobot envs, whose reference step has
no continuous `None`).  Here the population is the batch:
member k drives env k, all forwards are two batched matmuls on the stepper's own HIP stream (DeviceVecEnv, io_device = 1),
the int32 action tensor is read by the stepper in place, and the only host read is a `done.all()` every 16 steps.

The `cma` package is not available in this environment; the strategy itself — (mu/mu_w, lambda)-CMA-ES with cumulative
step-size adaptation and rank-one + rank-mu covariance updates, Hansen's tutorial parameter settings, i.e. what
`cma.CMAEvolutionStrategy(x0, sigma0, {'popsize': n})` runs — is restated in `CMAES` below as torch tensor code on the same
device.

--fused-rollout (off by default; the envs ARS fuses; ground-truth observations, --deterministic or --continuous-actions, no frame
stacking): one generation is reset + ONE srlhip_rollout_mlp_policy launch — the population, cast to float32 as the reference's torch
parameters are, is the kernel's parameter plane as it is, member k's MLP picks env k's actions inside the kernel — and the returns
come from the reward / done planes.  Softmax sampling (no --deterministic) stays on the per-step path unless --fused-sampling is given.

--fused-returns (off by default; needs --fused-rollout on ground-truth observations; ARS's rules: ARSModel.check_returns_arguments):
the launch returns each member's return and live-step count itself (srlhip_rollout_policy_summary) — the same generation, no planes.

--fused-sampling (off by default; needs --fused-rollout and discrete actions): the reference's default form — no --deterministic, each
member's action drawn from the softmax of its scores (cma_es.py:228-232) — in the same one launch (srlhip_rollout_mlp_policy_sampled).
The action draws then come from each env's own counter-based action stream (Philox stream 1, keyed by seed and env id), not from the
`torch.multinomial` generator of the per-step path: the two paths sample the same distribution but not the same bits.  (The reference
draws from the global np.random: no per-env stream could reproduce it either.)

A learned SRL model (--srl-model autoencoder, ...; SRLType.SRL) runs on every path: makeEnv builds a PixelStateVecEnv under the same
wrappers (ars.py: make_base_env), and --fused-rollout / --fused-sampling become T x (srlhip_policy_act, step + rasteriser, encoder)
on the env's stream (env.rollout_mlp_policy).

--cnn-policy (off by default; with --srl-model raw_pixels, --num-stack 1): the reference's default form — CNNPolicyPytorch on the frame
itself (cma_es.py:93-99,259-300), every member its own three-layer CNN whose batch-norm runs in training mode on the one frame it sees.
makeEnv builds a RawPixelVecEnv (no VecNormalize: the reference has none on raw pixels either, rl_baselines/utils.py:224), the CMA-ES
vector has cnn_param_count() entries, and member k's action for env k is ONE srlhip_cnn_policy_act launch on the frames where the
rasteriser left them: the argmax with --deterministic, a draw from the softmax with the env's own action stream by default, the score
row with --continuous-actions.  --fused-rollout (--fused-sampling included) enqueues the whole generation, T x (srlhip_cnn_policy_act,
step + rasteriser), with no host read in between (env.rollout_cnn_policy).  Without the flag raw_pixels is refused as before."""
import math
import pickle
import time

import numpy as np
import torch

from srlhip import _lib
from srlhip.device_env import DeviceVecEnv, DeviceVecFrameStack, DeviceVecNormalize, first_done_masks
from srlhip.envs import ENV_CLASSES
from rl_baselines.evolution_strategies.ars import ARSModel


class CMAES(object):
    """ask() -> [lambda, n] candidates; tell(candidates, losses) (minimisation).  float64 tensors on `device`."""

    def __init__(self, x0, sigma0, popsize, device, seed=0):
        n = len(x0)
        self.n, self.lam, self.device = n, int(popsize), device
        self.mean = torch.as_tensor(np.asarray(x0, dtype=np.float64), device=device)
        self.sigma = float(sigma0)
        self.mu = self.lam // 2
        w = math.log(self.mu + 0.5) - torch.log(torch.arange(1, self.mu + 1, dtype=torch.float64, device=device))
        self.weights = w / w.sum()
        self.mueff = float(1.0 / (self.weights ** 2).sum())
        self.cc = (4 + self.mueff / n) / (n + 4 + 2 * self.mueff / n)
        self.cs = (self.mueff + 2) / (n + self.mueff + 5)
        self.c1 = 2 / ((n + 1.3) ** 2 + self.mueff)
        self.cmu = min(1 - self.c1, 2 * (self.mueff - 2 + 1 / self.mueff) / ((n + 2) ** 2 + self.mueff))
        self.damps = 1 + 2 * max(0.0, math.sqrt((self.mueff - 1) / (n + 1)) - 1) + self.cs
        self.chiN = math.sqrt(n) * (1 - 1 / (4 * n) + 1 / (21 * n * n))
        self.pc = torch.zeros(n, dtype=torch.float64, device=device)
        self.ps = torch.zeros(n, dtype=torch.float64, device=device)
        self.C = torch.eye(n, dtype=torch.float64, device=device)
        self.B = torch.eye(n, dtype=torch.float64, device=device)
        self.D = torch.ones(n, dtype=torch.float64, device=device)
        self.gen, self.eigen_gen = 0, 0
        self.rng = torch.Generator(device=device)
        self.rng.manual_seed(int(seed))
        self.xbest, self.fbest = self.mean.clone(), float("inf")

    def ask(self):
        z = torch.randn((self.lam, self.n), dtype=torch.float64, device=self.device, generator=self.rng)
        self._y = (z * self.D) @ self.B.T                       # N(0, C)
        return self.mean + self.sigma * self._y

    def tell(self, x, losses):
        losses = torch.as_tensor(losses, dtype=torch.float64, device=self.device)
        order = torch.argsort(losses)
        if float(losses[order[0]]) < self.fbest:
            self.fbest, self.xbest = float(losses[order[0]]), x[order[0]].clone()
        y = self._y[order[:self.mu]]
        yw = (self.weights.unsqueeze(1) * y).sum(0)
        self.mean = self.mean + self.sigma * yw
        self.gen += 1
        invsqrtC_yw = self.B @ ((self.B.T @ yw) / self.D)
        self.ps = (1 - self.cs) * self.ps + math.sqrt(self.cs * (2 - self.cs) * self.mueff) * invsqrtC_yw
        hsig = float(self.ps.norm()) / math.sqrt(1 - (1 - self.cs) ** (2 * self.gen)) / self.chiN < 1.4 + 2 / (self.n + 1)
        self.pc = (1 - self.cc) * self.pc + (math.sqrt(self.cc * (2 - self.cc) * self.mueff) * yw if hsig else 0.0)
        rank_mu = (y.T * self.weights) @ y
        self.C = ((1 - self.c1 - self.cmu) * self.C + self.c1 * (torch.outer(self.pc, self.pc) + (0.0 if hsig else self.cc * (2 - self.cc)) * self.C)
                  + self.cmu * rank_mu)
        self.sigma *= math.exp((self.cs / self.damps) * (float(self.ps.norm()) / self.chiN - 1))
        if self.gen - self.eigen_gen > self.lam / ((self.c1 + self.cmu) * self.n * 10):      # O(n^2) amortised, as in the tutorial
            self.eigen_gen = self.gen
            self.C = torch.triu(self.C) + torch.triu(self.C, 1).T
            d, self.B = torch.linalg.eigh(self.C)
            self.D = torch.sqrt(torch.clamp(d, min=1e-20))


class BatchedMLP(object):
    """The reference's MLPPolicyPytorch(in, [100], out) for a whole population: parameters [P, n] in nn.Module.parameters()
    order (fc_in.weight [H, D], fc_in.bias [H], fc_out.weight [A, H], fc_out.bias [A]) -> scores [P, A]."""

    def __init__(self, in_dim, out_dim, hidden=100):
        self.D, self.H, self.A = int(in_dim), int(hidden), int(out_dim)
        self.n_params = self.H * self.D + self.H + self.A * self.H + self.A

    def split(self, params):
        D, H, A = self.D, self.H, self.A
        o = 0
        w1 = params[..., o:o + H * D].reshape(params.shape[:-1] + (H, D)); o += H * D
        b1 = params[..., o:o + H]; o += H
        w2 = params[..., o:o + A * H].reshape(params.shape[:-1] + (A, H)); o += A * H
        b2 = params[..., o:o + A]
        return w1, b1, w2, b2

    def forward(self, params, obs):
        """params [P, n], obs [P, D] -> [P, A]"""
        w1, b1, w2, b2 = self.split(params)
        h = torch.relu(torch.bmm(w1, obs.to(params.dtype).unsqueeze(-1)).squeeze(-1) + b1)
        return torch.bmm(w2, h.unsqueeze(-1)).squeeze(-1) + b2


class BatchedCNN(object):
    """The reference's CNNPolicyPytorch(C, A) on [H][W][C] frames, shape and host forward: parameters in nn.Module.parameters() order
    (conv1.weight [8][C][5][5], norm1.weight, norm1.bias, conv2.weight [16][8][3][3], norm2.*, conv3.weight [32][16][3][3], norm3.*,
    fc.weight [A][F], fc.bias [A]); F = 32 h3 w3 follows the frame size (288 at 224 x 224, the reference's constant).  The batch-norm is
    the reference's as it runs: training mode on one observation, i.e. every frame's own per-channel statistics."""
    CHANNELS = (8, 16, 32)

    def __init__(self, in_channels, img_h, img_w, out_dim):
        self.C, self.img_h, self.img_w, self.A = int(in_channels), int(img_h), int(img_w), int(out_dim)
        h, w = (self.img_h + 4 - 5) // 2 + 1, (self.img_w + 4 - 5) // 2 + 1
        for _ in range(2):
            h, w = (h // 2 + 2 - 3) // 2 + 1, (w // 2 + 2 - 3) // 2 + 1
        self.F = 32 * (h // 2) * (w // 2)
        assert self.F > 0, "frames of {} x {} leave nothing behind the third pool (sides 43..224)".format(img_h, img_w)
        self.blocks = [(8, self.C, 5, 5), (8,), (8,), (16, 8, 3, 3), (16,), (16,), (32, 16, 3, 3), (32,), (32,), (self.A, self.F), (self.A,)]
        self.n_params = int(sum(np.prod(b) for b in self.blocks))

    def split(self, params):
        out, o = [], 0
        for b in self.blocks:
            k = int(np.prod(b))
            out.append(params[o:o + k].reshape(b)); o += k
        return out

    def forward(self, params, frames):
        """params [n_params] (a float tensor), frames uint8 / float [B][H][W][C] -> scores [B][A]; every frame is normalised on its own"""
        w1, g1, b1, w2, g2, b2, w3, g3, b3, fw, fb = self.split(params)
        x = (torch.as_tensor(np.asarray(frames, dtype=np.float64) / 255.0)).permute(0, 3, 1, 2).to(params.dtype)
        for w, g, b, pad in ((w1, g1, b1, 2), (w2, g2, b2, 1), (w3, g3, b3, 1)):
            x = torch.nn.functional.conv2d(x, w, stride=2, padding=pad)
            mean, var = x.mean(dim=(2, 3), keepdim=True), x.var(dim=(2, 3), unbiased=False, keepdim=True)
            x = (x - mean) / torch.sqrt(var + 1e-5) * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
            x = torch.nn.functional.max_pool2d(torch.relu(x), 2)
        return x.reshape(x.shape[0], -1) @ fw.T + fb


class CMAESModel(object):
    def __init__(self):
        self.policy = None              # BatchedMLP (shape only; the parameters are best_model)
        self.n_population = None
        self.mu = None
        self.sigma = None
        self.continuous_actions = None
        self.deterministic = None
        self.es = None
        self.best_model = None          # numpy parameter vector of the best member seen (cma's result.xbest)

    def save(self, save_path, _locals=None):
        assert self.policy is not None, "Error: must train or load model before use"
        d = dict(self.__dict__)
        d["es"] = None                  # device tensors / generator stay out of the pickle
        with open(save_path, "wb") as f:
            pickle.dump(d, f)

    @classmethod
    def load(cls, load_path, args=None):
        with open(load_path, "rb") as f:
            class_dict = pickle.load(f)
        loaded_model = CMAESModel()
        loaded_model.__dict__ = class_dict
        return loaded_model

    def customArguments(self, parser):
        parser.add_argument('--num-population', help='Number of population', type=int, default=20)
        parser.add_argument('--mu', type=float, default=0, help='inital location for gaussian sampling of network parameters')
        parser.add_argument('--sigma', type=float, default=0.14, help='inital scale for gaussian sampling of network parameters')
        parser.add_argument('--cuda', action='store_true', default=False, help='use gpu for the neural network')
        parser.add_argument('--deterministic', action='store_true', default=False,
                            help='do a deterministic approach for the actions on the output of the policy')
        parser.add_argument('--fused-rollout', action='store_true', default=False,
                            help='evaluate each generation with one fused MLP-policy rollout launch (ground-truth observations or a learned SRL model; needs '
                                 '--deterministic or --continuous-actions and --num-stack 1; not KukaRandButton). The training '
                                 'callback then fires once per generation, not once per env step')
        parser.add_argument('--fused-sampling', action='store_true', default=False,
                            help='with --fused-rollout and discrete actions: draw each action from the softmax of the scores inside '
                                 'the fused launch (no --deterministic needed). The draws come from each env\'s own action stream, not '
                                 'from the torch.multinomial generator of the per-step path: same distribution, other bits')
        parser.add_argument('--fused-returns', action='store_true', default=False,
                            help='with --fused-rollout on ground-truth observations: the launch returns each member\'s return and live steps '
                                 'itself instead of the reward / done planes (same returns; not with a learned SRL model or --cnn-policy)')
        parser.add_argument('--cnn-policy', action='store_true', default=False,
                            help='with --srl-model raw_pixels: the reference\'s CNN-from-pixels policy, one network per member, run on '
                                 'the device from the rendered frames (srlhip_cnn_policy_act; --num-stack 1, frames of 43..224 a side)')
        return parser

    HIDDEN = 100                        # MLPPolicyPytorch(obs_dim, [100], n_actions)

    # --fused-rollout: the episode limits are ARS's, and so are the argument rules behind CMA-ES's own for --fused-sampling
    FUSED_EPISODE_LIMIT = ARSModel.FUSED_EPISODE_LIMIT

    @staticmethod
    def check_fused_arguments(args):
        """--fused-sampling against the rest of the arguments, then ARS's rules for --fused-rollout, whose "--deterministic or
        --continuous-actions" requirement --fused-sampling meets; raises ValueError before any env is built.  --fused-returns is
        checked first (ARSModel.check_returns_arguments)."""
        ARSModel.check_returns_arguments(args)
        if CMAESModel.cnn_from_pixels(args):
            # the CNN-from-pixels path: every action selection has a fused form (the loop of launches samples as the per-step path does)
            if int(getattr(args, "num_stack", 1)) != 1:
                raise ValueError("--cnn-policy needs --num-stack 1: the CNN reads one frame")
            if getattr(args, "fused_sampling", False) and not getattr(args, "fused_rollout", False):
                raise ValueError("--fused-sampling needs --fused-rollout")
            if getattr(args, "fused_sampling", False) and getattr(args, "continuous_actions", False):
                raise ValueError("--fused-sampling needs discrete actions (not --continuous-actions): continuous actions are never sampled")
            return
        if not getattr(args, "fused_sampling", False):
            return ARSModel.check_fused_arguments(args)
        if not getattr(args, "fused_rollout", False):
            raise ValueError("--fused-sampling needs --fused-rollout")
        if getattr(args, "continuous_actions", False):
            raise ValueError("--fused-sampling needs discrete actions (not --continuous-actions): continuous actions are never sampled")
        met = type(args)(**dict(vars(args), deterministic=True))       # ARS's rules with that one requirement met
        return ARSModel.check_fused_arguments(met)

    @staticmethod
    def cnn_from_pixels(args):
        return bool(getattr(args, "cnn_policy", False)) and getattr(args, "srl_model", "ground_truth") == "raw_pixels"

    @staticmethod
    def returns_from_planes(reward, done):
        """The reference's accounting (cma_es.py:127-133) on [T][N] reward / done planes -> (float64 returns [N], int64 live steps
        [N]).  `r[~done] += reward` runs AFTER `done` is updated, so the reward of a member's finishing step is not added; `step +=
        sum(~done)` runs before the step, so a member's live steps are the rows up to and including its first done."""
        seen, before = first_done_masks(done)
        ret = (reward.to(torch.float64) * (~seen).to(torch.float64)).sum(0)
        return ret, (~before).to(torch.int64).sum(0)

    def evaluate_fused(self, env, population, T):
        """One generation in one launch (the env was just reset): member k's MLP drives env k, frozen after its first done ->
        (r [P] float64, live_steps [P] int64).  A model that is neither deterministic nor continuous samples its actions (the
        argument rules have asked for --fused-sampling)."""
        sample = self.deterministic is False and not self.continuous_actions       # (None, a model train() has not configured: the argmax)
        kw = {"sample": True} if sample else {}
        if isinstance(self.policy, BatchedCNN):
            planes = env.rollout_cnn_policy(T, population.to(torch.float32).contiguous(), per_env=True, freeze_after_done=True, sample=sample)
            return self.returns_from_planes(planes["reward"], planes["done"])
        if getattr(self, "fused_returns", False):          # --fused-returns: the launch reduces; moments only where a wrapper wants them
            out = env.rollout_mlp_policy_summary(T, population.to(torch.float32).contiguous(), self.policy.H, per_env=True, freeze_after_done=True,
                                                 moments=False, **kw)
            return out["ret"], out["length"].to(torch.int64)
        planes = env.rollout_mlp_policy(T, population.to(torch.float32).contiguous(), self.policy.H, per_env=True, freeze_after_done=True, **kw)
        return self.returns_from_planes(planes["reward"], planes["done"])

    @classmethod
    def getOptParam(cls):
        return {"sigma": (float, (0, 0.2))}

    # ---- host-side single-policy interface (replay / enjoy) ----------------------------------------------------------
    def _scores(self, observation):
        assert self.policy is not None and self.best_model is not None, "Error: must train or load model before use"
        if isinstance(self.policy, BatchedCNN):          # frames [B][H][W][C] (or one frame): obs / 255.0, NHWC -> NCHW as the reference does
            frames = np.asarray(observation)
            frames = frames[None] if frames.ndim == 3 else frames
            # the parameters as the device (and the reference's toTensor) holds them: float32; the forward itself in float64
            return self.policy.forward(torch.as_tensor(np.asarray(self.best_model, dtype=np.float32)).double(), frames).numpy()
        obs = torch.as_tensor(np.atleast_2d(np.asarray(observation, dtype=np.float64)))
        params = torch.as_tensor(self.best_model, dtype=torch.float64).unsqueeze(0).expand(len(obs), -1)
        return self.policy.forward(params, obs).numpy()

    def getActionProba(self, observation, dones=None):
        scores = self._scores(observation)
        if self.continuous_actions:
            return scores
        z = np.exp(scores - scores.max(axis=1, keepdims=True))
        return z / z.sum(axis=1, keepdims=True)

    def getAction(self, observation, dones=None):
        if self.continuous_actions:
            return self._scores(observation)
        if self.deterministic:
            return self._scores(observation).argmax(axis=1)
        cdf = np.cumsum(self.getActionProba(observation), axis=1)
        return (np.random.random_sample((len(cdf), 1)) * cdf[:, -1:] < cdf).argmax(axis=1)

    # ---- env assembly: cma_es.py:79-80 (createEnvs with allow_early_resets) on the device-resident stack ----------------
    @classmethod
    def makeEnv(cls, args, env_kwargs=None, load_path_normalise=None):
        env_kwargs = dict(env_kwargs or {})
        env_kwargs.setdefault("srl_model", getattr(args, "srl_model", "ground_truth"))
        if env_kwargs["srl_model"] == "raw_pixels":
            if not getattr(args, "cnn_policy", False):
                raise NotImplementedError("CMA-ES on the device stack evaluates state policies (MLP); the reference's CNN-from-pixels "
                                          "policy is not part of it unless --cnn-policy is given")
            if int(getattr(args, "num_stack", 1)) != 1:
                raise ValueError("--cnn-policy needs --num-stack 1: the CNN reads one frame")
            from srlhip.pixel_env import RawPixelVecEnv
            from srlhip.vec_env import RNG_MODES, default_rng_mode
            img_shape = tuple(env_kwargs.get("img_shape") or getattr(args, "img_shape", None) or (224, 224))[-2:]
            return RawPixelVecEnv(args.env, args.num_cpu, seed=args.seed, img_shape=img_shape, device_id=getattr(args, "device_id", 0),
                                  rng_mode=RNG_MODES[default_rng_mode("device")], env_kwargs=env_kwargs)
        envs = ARSModel.make_base_env(args, env_kwargs)
        envs = DeviceVecFrameStack(envs, getattr(args, "num_stack", 1))
        envs = DeviceVecNormalize(envs, norm_obs=True, norm_reward=False)
        if load_path_normalise is not None:
            envs.training = False
            envs.load_running_average(load_path_normalise)
        return envs

    def train(self, args, callback=None, env_kwargs=None, train_kwargs=None):
        args.num_cpu = args.num_population
        merged = dict(vars(args), **(train_kwargs or {}))
        self.check_fused_arguments(type(args)(**merged))          # at argument time: before any env is built
        env = self.makeEnv(args, env_kwargs=env_kwargs)
        args.__dict__.update(train_kwargs or {})
        fused = bool(getattr(args, "fused_rollout", False))
        fused_T = self.FUSED_EPISODE_LIMIT.get(ENV_CLASSES[args.env].ENV_KIND, 0) + 1
        continuous = bool(getattr(args, "continuous_actions", False))
        none_rows = continuous and ENV_CLASSES[args.env].ENV_KIND >= _lib.ENV_KUKA_BUTTON      # finished members: `None` (Kuka)
        action_space = int(np.prod(env.action_space.shape)) if continuous else env.action_space.n
        cnn = self.cnn_from_pixels(args)
        if cnn:
            img_h, img_w, channels = env.observation_space.shape
            self.policy = BatchedCNN(channels, img_h, img_w, action_space)
            assert self.policy.n_params == env.cnn_param_count(), (self.policy.n_params, env.cnn_param_count())
        else:
            self.policy = BatchedMLP(int(np.prod(env.observation_space.shape)), action_space, self.HIDDEN)
        self.n_population, self.mu, self.sigma = args.num_population, args.mu, args.sigma
        self.continuous_actions, self.deterministic = continuous, bool(getattr(args, "deterministic", False))
        self.fused_returns = bool(getattr(args, "fused_returns", False))
        P, dev = self.n_population, env.device
        self.es = CMAES(self.policy.n_params * [self.mu], self.sigma, P, dev, seed=int(args.seed))
        self.best_model = np.array(self.policy.n_params * [self.mu], dtype=np.float64)
        num_updates = int(args.num_timesteps)
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(args.seed) + 1)
        start_time, step = time.time(), 0
        self.history = []
        log_dir = getattr(args, "log_dir", None)
        with torch.cuda.stream(env.torch_stream):          # policy math and stepper kernels on ONE stream: no host syncs
            while step < num_updates:
                obs = env.reset()
                population = self.es.ask()                  # [P, n_params]
                live = torch.zeros((), dtype=torch.int64, device=dev)
                if fused:                                   # one launch
                    r, live_steps = self.evaluate_fused(env, population, fused_T)
                    live += live_steps.sum()
                    if callback is not None:
                        callback(locals(), globals())       # once per generation on this path
                else:                                       # the per-step path
                    r = torch.zeros(P, dtype=torch.float64, device=dev)
                    done = torch.zeros(P, dtype=torch.bool, device=dev)
                    k = 0
                    params32 = population.to(torch.float32).contiguous() if cnn else None
                    while True:
                        if cnn:                                 # one launch: member k's CNN on env k's frame, the selection included
                            picked = env.cnn_policy_act(params32, per_env=True, sample=not (continuous or self.deterministic))
                        scores = picked if cnn else self.policy.forward(population, obs)      # (continuous: the CNN's row IS the scores)
                        if none_rows:
                            actions = torch.where(done.unsqueeze(-1), torch.full_like(scores, float("nan")), scores).to(torch.float32).contiguous()
                        elif continuous:
                            actions = (scores * (~done).unsqueeze(-1).to(scores.dtype)).to(torch.float32).contiguous()
                        else:
                            a = picked if cnn else torch.argmax(scores, dim=1) if self.deterministic else \
                                torch.multinomial(torch.softmax(scores, dim=1), 1, generator=gen).squeeze(1)
                            actions = torch.where(done, torch.full_like(a, -1), a).to(torch.int32).contiguous()      # None: "do nothing, as we are done"
                        live += (~done).sum()                   # step += np.sum(~done) (cma_es.py:127)
                        obs, reward, new_done = env.step(actions)
                        done = done | (new_done != 0)
                        r += reward.to(torch.float64) * (~done).to(torch.float64)      # cumulate the reward of every member that is not finished
                        k += 1
                        if callback is not None:
                            callback(locals(), globals())
                        if k % 16 == 0 and bool(done.all()):    # the only device->host read
                            break
                step += int(live)
                print("{} steps - {:.2f} FPS".format(step, step / (time.time() - start_time)))
                self.es.tell(population, -r)
                self.best_model = self.es.xbest.cpu().numpy()
                self.history.append(float(r.mean()))
        if log_dir is not None and hasattr(env, "save_running_average"):
            env.save_running_average(log_dir)
        env.close()
        return self
