"""Train srl_zoo's linear state encoder on a recorded dataset — the model SRLLinear (state_representation/models.py) applies.

In the reference a learned state model comes out of srl_zoo (an empty submodule of the reference checkout) as a checkpoint nobody here
can produce; this module trains the smallest member of that family, `--model-type linear`, state = fc(flatten(preprocess(frame))), so
that record -> TRAIN -> evaluate -> RL closes for a learned model: `dataset_generator` records, this module writes `srl_model.pth` +
`exp_config.json`, `--srl-model inverse` (or any other name whose path points there) loads them through loadSRLModel unchanged.

THE LOSSES [recalled from srl_zoo, UNVERIFIED: its code cannot be read here], each with a weight (default 1):
  supervised  MSE of the state against the ground truth; the state dimension is the ground truth's.  Alone it is the reference's
              supervised baseline: the checkpoint is a bare module under baselines/supervised_linear_ST_DIM<k>/srl_supervised_model.pth.
  inverse     cross-entropy of the action a_t from a linear head on [s_t, s_t+1].
  forward     MSE of s_t+1 against s_t + Linear([s_t, onehot(a_t)]).
Pairs (t, t + 1) that cross an episode start are dropped.

ONE TRAINING STEP.  The encoder's parameters are V float64 [F][S] (F in the frame's own NHWC order) and c [S]; the heads and c are float64
torch parameters under torch.optim.Adam.  forward on the batch's frames (srlhip_linear_srl_forward) -> the states as a leaf tensor with
requires_grad -> the torch loss and backward() -> G = states.grad -> srlhip_linear_srl_step: gradient frames^T G and the Adam update of V
in ONE launch on the same stream (csrc/linear_srl.hip; the contract is in include/srlhip.h).  No float64 copy of the frames, no [F][S]
gradient, no host read inside an epoch.
BACKENDS.  "hip": the two kernels.  "host": their twins through ctypes (the same header functions: the same bits in V after any number
of steps, given the same G).  "torch": the plain formulation — a float64 copy of the frames, matmul, autograd, torch.optim.Adam on V —
which runs on a CPU and is what the others are compared with.  "auto": hip where a GPU is visible, else host.

    python -m state_representation.linear_srl --data-folder D --state-dim K --losses inverse forward --log-folder OUT
        [--epochs 10] [--batch-size 256] [--learning-rate 1e-3] [--seed 0] [--backend auto|hip|host|torch] [--device-id 0]
        [--decode-backend pillow|hip|auto|hip-baseline] [--evaluate] [--supervised-weight 1] [--inverse-weight 1] [--forward-weight 1]
"""
import argparse
import json
import os

import numpy as np

from state_representation.models import linear_tables, linear_to_checkpoint

LOSSES = ("supervised", "inverse", "forward")
MAX_BATCH_FRAMES = 1024                   # srlhip_linear_srl_*: frames per call
BETAS, EPS = (0.9, 0.999), 1e-8           # torch.optim.Adam's defaults, for V as for the heads


def resolve_backend(backend):
    import torch
    if backend not in ("auto", "hip", "host", "torch"):
        raise ValueError("backend must be auto, hip, host or torch")
    if backend == "auto":
        backend = "hip" if torch.cuda.is_available() else "host"
    if backend == "hip" and not torch.cuda.is_available():
        raise RuntimeError("backend='hip' needs a GPU")
    return backend


class LinearEncoder(object):
    """V [F][S], c [S] and V's Adam moments on one backend.  forward(frames) -> float64 states [n][S] (a tensor on the backend's device,
    no autograd history on hip / host); step(frames, G) applies one Adam step to V from dL/dstates = G.  c is a torch parameter of the
    caller's optimiser on every backend; on "torch" V is one too (self.V_param) and step() only checks that it is not called."""

    def __init__(self, img_shape, n_channels, state_dim, backend="auto", device_id=0, learning_rate=1e-3, seed=0):
        import torch
        from srlhip import _lib
        self.backend = resolve_backend(backend)
        self.img_shape, self.n_channels, self.state_dim = tuple(img_shape), int(n_channels), int(state_dim)
        self.F = self.img_shape[0] * self.img_shape[1] * self.n_channels
        if not _lib.linear_srl_supported(self.F, self.state_dim, self.n_channels):
            raise ValueError("linear encoder: {} features, {} state dimensions, {} channels (F >= 1, 1 <= S <= 64, 1 <= C <= 8)".format(
                self.F, self.state_dim, self.n_channels))
        self.lr, self.t = float(learning_rate), 0
        self.scale, self.offset = linear_tables(self.n_channels)
        self.device = torch.device("cuda", device_id) if self.backend == "hip" or (self.backend == "torch" and torch.cuda.is_available()) \
            else torch.device("cpu")
        rng = np.random.RandomState(seed)
        bound = 1.0 / np.sqrt(self.F)                                       # nn.Linear's default initialisation range
        V = rng.uniform(-bound, bound, size=(self.F, self.state_dim))
        c = rng.uniform(-bound, bound, size=self.state_dim)
        self.c = torch.nn.Parameter(torch.from_numpy(c).to(self.device))
        self._lib = _lib
        if self.backend == "host":
            self.V, self.m, self.v = V, np.zeros_like(V), np.zeros_like(V)
        elif self.backend == "hip":
            self.V = torch.from_numpy(V).to(self.device)
            self.m, self.v = torch.zeros_like(self.V), torch.zeros_like(self.V)
            self._work = None
        else:
            self.V_param = torch.nn.Parameter(torch.from_numpy(V).to(self.device))
            ch = np.arange(self.F) % self.n_channels
            self._scale_f = torch.from_numpy(self.scale[ch]).to(self.device)
            self._offset_f = torch.from_numpy(self.offset[ch]).to(self.device)

    def _frames(self, frames):
        import torch
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        n = int(frames.shape[0])
        assert frames.dtype == torch.uint8 and 1 <= n <= MAX_BATCH_FRAMES, (frames.dtype, n)
        frames = frames.reshape(n, -1)
        assert frames.shape[1] == self.F, frames.shape
        return frames.to(self.device).contiguous(), n

    def forward(self, frames):
        import torch
        x, n = self._frames(frames)
        if self.backend == "torch":
            return torch.addmm(self.c, x.to(torch.float64) * self._scale_f - self._offset_f, self.V_param)
        if self.backend == "host":
            return torch.from_numpy(self._lib.linear_srl_forward_host(x.numpy(), self.scale, self.offset, self.V, self.c.detach().numpy()))
        need = self._lib.linear_srl_workspace_bytes(self.F, self.state_dim, n)
        if self._work is None or self._work.numel() * 8 < need:
            self._work = torch.empty(((need + 7) // 8,), dtype=torch.float64, device=self.device)
        states = torch.empty((n, self.state_dim), dtype=torch.float64, device=self.device)
        self._lib.linear_srl_forward(self.device.index, x.data_ptr(), n, self.F, self.state_dim, self.scale, self.offset, self.V.data_ptr(),
                                     self.c.data_ptr(), states.data_ptr(), self._work.data_ptr(),
                                     stream=torch.cuda.current_stream(self.device).cuda_stream)
        return states

    def step(self, frames, G, grad_out=None):
        """one Adam step of V from G = dL/dstates [n][S] of these frames (hip: a device tensor; host: anything numpy reads)"""
        import torch
        assert self.backend != "torch", "on the torch backend V belongs to the caller's optimiser"
        x, n = self._frames(frames)
        self.t += 1
        adam = self._lib.adam_at(self.t, self.lr, BETAS[0], BETAS[1], EPS)
        if self.backend == "host":
            G = np.ascontiguousarray(G.detach().cpu().numpy() if isinstance(G, torch.Tensor) else G, dtype=np.float64)
            self._lib.linear_srl_step_host(x.numpy(), self.scale, self.offset, G, self.V, self.m, self.v, adam, grad_out)
            return
        G = (G if isinstance(G, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(G))).to(self.device, torch.float64).contiguous()
        assert tuple(G.shape) == (n, self.state_dim), G.shape
        self._lib.linear_srl_step(self.device.index, x.data_ptr(), n, self.F, self.state_dim, self.scale, self.offset, G.data_ptr(),
                                  self.V.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), adam,
                                  grad_out_ptr=None if grad_out is None else grad_out.data_ptr(),
                                  stream=torch.cuda.current_stream(self.device).cuda_stream)

    def weights(self):
        """-> (V [F][S], c [S]) as numpy float64"""
        V = self.V_param.detach().cpu().numpy() if self.backend == "torch" else self.V if self.backend == "host" else self.V.cpu().numpy()
        return np.array(V, dtype=np.float64), self.c.detach().cpu().numpy().astype(np.float64)


class LinearSRLTrainer(object):
    """The encoder, the loss heads and their optimiser.  losses: a subset of LOSSES in the caller's order (it is written to exp_config.json
    as given); weights: {loss: weight}."""

    def __init__(self, img_shape, n_channels, state_dim, losses, n_actions, backend="auto", device_id=0, learning_rate=1e-3, seed=0, weights=None):
        import torch
        losses = list(losses)
        if not losses or any(name not in LOSSES for name in losses) or len(set(losses)) != len(losses):
            raise ValueError("losses: a non-empty subset of {} (got {})".format(LOSSES, losses))
        self.losses, self.n_actions = losses, int(n_actions)
        self.weights = dict({name: 1.0 for name in LOSSES}, **(weights or {}))
        self.pairs = "inverse" in losses or "forward" in losses
        if self.pairs and self.n_actions < 1:
            raise ValueError("the inverse and forward losses need discrete actions (n_actions >= 1)")
        self.encoder = LinearEncoder(img_shape, n_channels, state_dim, backend, device_id, learning_rate, seed)
        enc, S = self.encoder, int(state_dim)
        torch.manual_seed(int(seed))                                        # the heads' initialisation (made on the CPU, then moved)
        self.inverse_net = torch.nn.Linear(2 * S, self.n_actions).double().to(enc.device) if "inverse" in losses else None
        self.forward_net = torch.nn.Linear(S + self.n_actions, S).double().to(enc.device) if "forward" in losses else None
        params = [enc.c] + [p for net in (self.inverse_net, self.forward_net) if net is not None for p in net.parameters()]
        if enc.backend == "torch":
            params.append(enc.V_param)
        self.optimizer = torch.optim.Adam(params, lr=float(learning_rate), betas=BETAS, eps=EPS)

    def loss(self, states, n_pairs, actions, ground_truth):
        """states [n][S] in the autograd graph: rows 0 .. n_pairs - 1 are s_t and, with a pair loss, rows n_pairs .. 2 n_pairs - 1 s_t+1"""
        import torch
        import torch.nn.functional as Fn
        s_t = states[:n_pairs]
        total = states.new_zeros(())
        if "supervised" in self.losses:
            total = total + self.weights["supervised"] * Fn.mse_loss(s_t, ground_truth)
        if self.pairs:
            s_next = states[n_pairs:2 * n_pairs]
            if "inverse" in self.losses:
                total = total + self.weights["inverse"] * Fn.cross_entropy(self.inverse_net(torch.cat([s_t, s_next], dim=1)), actions)
            if "forward" in self.losses:
                onehot = Fn.one_hot(actions, self.n_actions).to(torch.float64)
                total = total + self.weights["forward"] * Fn.mse_loss(s_t + self.forward_net(torch.cat([s_t, onehot], dim=1)), s_next)
        return total

    def train_step(self, frames, n_pairs, actions=None, ground_truth=None):
        """frames uint8 [n_pairs or 2 n_pairs][...] -> the loss (a 0-d tensor on the device: nothing is read back here)"""
        enc = self.encoder
        self.optimizer.zero_grad(set_to_none=True)
        if enc.backend == "torch":
            total = self.loss(enc.forward(frames), n_pairs, actions, ground_truth)
            total.backward()
            self.optimizer.step()
            return total.detach()
        leaf = enc.forward(frames).requires_grad_(True)
        # (c went into the states inside the kernel: adding c - c.detach(), an exact zero, gives it its gradient, the column sums of G)
        total = self.loss(leaf + (enc.c - enc.c.detach()), n_pairs, actions, ground_truth)
        total.backward()
        enc.step(frames, leaf.grad)
        self.optimizer.step()
        return total.detach()

    def fit(self, frames, actions=None, episode_starts=None, ground_truth=None, epochs=10, batch_size=256, seed=0):
        """frames uint8 [N][H][W][C] in recording order (numpy or a device tensor) -> the mean loss of every epoch (read back once per
        epoch).  With a pair loss a batch is batch_size transitions: 2 batch_size frames go through the encoder."""
        import torch
        enc = self.encoder
        N = int(frames.shape[0])
        frames = (torch.from_numpy(np.ascontiguousarray(frames)) if isinstance(frames, np.ndarray) else frames).to(enc.device)
        if self.pairs:
            starts = np.asarray(episode_starts).astype(bool).reshape(-1)
            assert len(starts) == N and len(actions) == N, "actions and episode_starts have one row per frame"
            index = np.flatnonzero(~starts[1:])                             # t with t + 1 inside the same episode
            actions = torch.from_numpy(np.asarray(actions).reshape(-1).astype(np.int64)).to(enc.device)
        else:
            index = np.arange(N)
        if "supervised" in self.losses:
            ground_truth = torch.from_numpy(np.asarray(ground_truth, dtype=np.float64).reshape(N, -1)).to(enc.device)
            assert ground_truth.shape[1] == enc.state_dim, "the supervised loss needs state_dim = the ground truth's dimension"
        batch_size = int(batch_size)
        if not 1 <= batch_size * (2 if self.pairs else 1) <= MAX_BATCH_FRAMES:
            raise ValueError("batch_size: 1..{} ({} frames per call)".format(MAX_BATCH_FRAMES // (2 if self.pairs else 1), MAX_BATCH_FRAMES))
        if len(index) == 0:
            raise ValueError("no training samples in the dataset")
        rng = np.random.RandomState(seed)
        history = []
        for _ in range(int(epochs)):
            order = torch.from_numpy(index[rng.permutation(len(index))]).to(enc.device)
            total = torch.zeros((), dtype=torch.float64, device=enc.device)
            for b in range(0, len(order), batch_size):
                t = order[b:b + batch_size]
                batch = frames[torch.cat([t, t + 1])] if self.pairs else frames[t]
                total += self.train_step(batch, len(t), actions[t] if self.pairs else None,
                                         ground_truth[t] if "supervised" in self.losses else None) * len(t)
            history.append(float(total) / len(order))                       # the epoch's one host read
        return history

    def save(self, log_folder):
        """-> the checkpoint's path.  SRLModules' key layout [recalled]: model.fc.weight [S][F'] (F' in the reference's C, W, H flatten
        order), model.fc.bias, inverse_net.*, forward_net.*; the supervised baseline alone is a bare module under baselines/."""
        import torch
        enc = self.encoder
        V, c = enc.weights()
        fc = {"fc.weight": torch.from_numpy(linear_to_checkpoint(V, enc.img_shape, enc.n_channels)), "fc.bias": torch.from_numpy(c)}
        if self.losses == ["supervised"]:
            out = os.path.join(log_folder, "baselines", "supervised_linear_ST_DIM{}".format(enc.state_dim))
            path, state = os.path.join(out, "srl_supervised_model.pth"), fc
        else:
            out = log_folder
            path, state = os.path.join(out, "srl_model.pth"), {"model." + k: v for k, v in fc.items()}
            for name, net in (("inverse_net", self.inverse_net), ("forward_net", self.forward_net)):
                if net is not None:
                    state.update({name + "." + k: v.detach().cpu() for k, v in net.state_dict().items()})
        os.makedirs(out, exist_ok=True)
        torch.save(state, path)
        with open(os.path.join(out, "exp_config.json"), "w") as f:
            json.dump({"state-dim": enc.state_dim, "losses": self.losses, "n_actions": self.n_actions, "model-type": "linear",
                       "inverse-model-type": "linear", "split-dimensions": -1, "multi-view": enc.n_channels == 6,
                       "img-shape": list(enc.img_shape), "backend": enc.backend}, f, indent=2)
        return path


def load_dataset(data_folder, decode_backend="pillow", device_id=0):
    """-> (frames uint8 [N][H][W][3] in ground_truth.npz's order, indices, actions, episode_starts, ground_truth_states): EVERY frame
    (pairs need consecutive ones)"""
    from state_representation import evaluate
    paths, indices = evaluate.dataset_items(data_folder, max_frames=2 ** 62)
    frames = evaluate.decode_items(paths, decode_backend, device_id)
    with np.load(os.path.join(data_folder, "preprocessed_data.npz")) as pp:
        actions, starts = np.asarray(pp["actions"]), np.asarray(pp["episode_starts"])
    with np.load(os.path.join(data_folder, "ground_truth.npz"), allow_pickle=True) as gt:
        truth = np.asarray(gt["ground_truth_states"], dtype=np.float64)
    return frames, indices, actions, starts, truth


def main(argv=None):
    parser = argparse.ArgumentParser(description="Train the linear SRL encoder on a recorded dataset")
    parser.add_argument("--data-folder", required=True, help="a dataset written by environments.dataset_generator")
    parser.add_argument("--state-dim", type=int, default=None, help="(the supervised loss alone: the ground truth's dimension)")
    parser.add_argument("--losses", nargs="+", default=["inverse", "forward"], choices=LOSSES)
    parser.add_argument("--log-folder", required=True, help="srl_model.pth and exp_config.json go here")
    parser.add_argument("--epochs", type=int, default=10)
    parser.add_argument("--batch-size", type=int, default=256)
    parser.add_argument("--learning-rate", type=float, default=1e-3)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--n-actions", type=int, default=None, help="(default: the largest recorded action + 1)")
    parser.add_argument("--device-id", type=int, default=0)
    parser.add_argument("--backend", default="auto", choices=("auto", "hip", "host", "torch"))
    parser.add_argument("--decode-backend", default="pillow", choices=("pillow", "hip", "auto", "hip-baseline"))
    for name in LOSSES:
        parser.add_argument("--{}-weight".format(name), type=float, default=1.0)
    parser.add_argument("--evaluate", action="store_true", default=False,
                        help="score the saved model on the frames it was trained on (state_representation.evaluate: knn_mse.json next to the model)")
    args = parser.parse_args(argv)
    frames, indices, actions, starts, truth = load_dataset(args.data_folder, args.decode_backend, args.device_id)
    truth = truth.reshape(len(truth), -1)
    state_dim = args.state_dim if args.state_dim is not None else (truth.shape[1] if "supervised" in args.losses else None)
    if state_dim is None:
        parser.error("--state-dim is required")
    n_actions = args.n_actions if args.n_actions is not None else int(np.asarray(actions).max()) + 1
    trainer = LinearSRLTrainer(tuple(frames.shape[1:3]), int(frames.shape[3]), state_dim, args.losses, n_actions, backend=args.backend,
                               device_id=args.device_id, learning_rate=args.learning_rate, seed=args.seed,
                               weights={name: getattr(args, name + "_weight") for name in LOSSES})
    history = trainer.fit(frames, actions, starts, truth, epochs=args.epochs, batch_size=args.batch_size, seed=args.seed)
    path = trainer.save(args.log_folder)
    print("trained {} on {} frames of {} ({}): loss {:.6g} -> {:.6g} over {} epochs -> {}".format(
        "+".join(args.losses), len(frames), "x".join(str(d) for d in frames.shape[1:]), trainer.encoder.backend, history[0], history[-1],
        len(history), path))
    if args.evaluate:
        from state_representation import evaluate
        backend = trainer.encoder.backend if trainer.encoder.backend in ("hip", "host") else "auto"
        out = evaluate.evaluate_model(args.data_folder, path, backend=backend, device_id=args.device_id, log_folder=os.path.dirname(path),
                                      frames=frames, indices=indices)
        print("knn_mse {:.6g} (k = {}, {} queries; ground truth as states {:.6g}), gtc_mean {:.4f}".format(
            out["knn_mse"], out["k"], out["n_queries"], out["knn_mse_ground_truth"], out["gtc_mean"]))
    return path


if __name__ == "__main__":
    main()
