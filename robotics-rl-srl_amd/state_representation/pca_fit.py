"""Fit the PCA state baseline from recorded frames — the model SRLPCA (state_representation/models.py) applies.

In the reference a PCA model comes out of srl_zoo (an empty submodule of the reference checkout) as a pickled sklearn object; here it is
fitted in the repository, so that record -> fit -> train closes: `dataset_generator` records frames, this module turns them into
`baselines/pca_ST_DIM<k>/pca.pkl` + `exp_config.json`, and `--srl-model pca` loads that through loadSRLModel unchanged.

The fit is the Gram ("dual") form of PCA, N frames of F features with N <= 8192 << F:
  a. gram = X X^T (int64 [N][N]) and its inputs' row sums, EXACT integers: on the device srlhip_pca_gram — the int8 matrix pipe on the
     frames' own bytes, no float64 copy of the frames — or on the host its twin (csrc/pca_gram.hpp has the contract).
  b. on the host, numpy: the exact integer centring M = N^2 gram - N R_i - N R_j + S (R the row sums of gram, S their sum: M / N^2 is the
     Gram matrix of the centred frames), C = float64(M) / float64(N^2), numpy.linalg.eigh(C), the top state_dim pairs in descending
     order, each u_k's sign fixed so that its largest-magnitude entry (the lowest index on a tie) is positive [sklearn's svd_flip
     convention, recalled].
  c. mean_ = column sums (exact int64) / N.
  d. components_ = (Xc^T u_k / sqrt(lam_k))^T through the EXISTING projection contract (srlhip_pca_forward / srlhip_pca_project_host: the
     transposed frames as F "frames" of N "features", W = U / sqrt(lam), b = 0), then - mean_ (1^T W) in numpy.
  e. explained_variance_ = lam / (N - 1), singular_values_ = sqrt(lam), whiten = False.
Step a is bit-identical between the backends because it is integer arithmetic, step d because the projection kernel equals its host twin
bit for bit, and everything else is the same numpy code: fit_pca(backend="hip") and fit_pca(backend="host") give the same bits.

    python -m state_representation.pca_fit --data-folder <recorded dataset> --state-dim K [--max-frames 4096] [--device-id 0] --log-folder <out>
        [--decode-backend hip]    (datasets of `dataset_generator --device-jpeg`: the files are decoded on the GPU and never exist decoded on the host)
        [--decode-backend hip-baseline]    (the same for datasets of the default recorder, Pillow's or OpenCV's files)
        [--evaluate]    (score the saved model on the frames it was fitted on: state_representation/evaluate.py, KNN-MSE and ground-truth
                         correlation into <log-folder>/baselines/pca_ST_DIM<k>/knn_mse.json)
"""
import argparse
import glob
import json
import os
import pickle

import numpy as np

MAX_FRAMES, MAX_DIM = 8192, 64


class FittedPCA(object):
    """What SRLPCA.set_model reads of a fitted sklearn PCA (components_ [k][F], mean_ [F], explained_variance_ [k], whiten), as a plain
    picklable object: the model loads where sklearn is absent."""

    def __init__(self, components, mean, explained_variance, singular_values, explained_variance_ratio, n_samples, backend):
        self.components_ = components
        self.mean_ = mean
        self.explained_variance_ = explained_variance
        self.explained_variance_ratio_ = explained_variance_ratio
        self.singular_values_ = singular_values
        self.whiten = False
        self.n_components = self.n_components_ = int(components.shape[0])
        self.n_features_ = self.n_features_in_ = int(components.shape[1])
        self.n_samples_ = int(n_samples)
        self.backend = backend

    def transform(self, X):
        X = np.asarray(X)
        return (X.reshape(len(X), -1).astype(np.float64) - self.mean_) @ self.components_.T

    def save(self, folder):
        """-> the path of <folder>/baselines/pca_ST_DIM<k>/pca.pkl (the reference's config/srl_models.yaml layout, which loadSRLModel
        recognises as a PCA model), with the exp_config.json it reads next to it"""
        out = os.path.join(folder, "baselines", "pca_ST_DIM{}".format(self.n_components_))
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "pca.pkl")
        with open(path, "wb") as f:
            pickle.dump(self, f, protocol=2)
        with open(os.path.join(out, "exp_config.json"), "w") as f:
            json.dump({"state-dim": self.n_components_, "model-type": "pca", "n-samples": self.n_samples_}, f, indent=2)
        return path


def centred_gram(gram):
    """int64 gram [N][N] of the raw frames -> float64 Gram matrix of the centred frames, from the exact integer N^2 (Xc Xc^T)"""
    N = gram.shape[0]
    R = gram.sum(axis=1)
    M = N * N * gram - N * R[:, None] - N * R[None, :] + R.sum()
    return M.astype(np.float64) / np.float64(N * N)


def top_pairs(C, state_dim):
    """-> (lam [k] descending, U [N][k]) of the symmetric C, signs fixed"""
    lam, U = np.linalg.eigh(C)
    lam, U = lam[::-1][:state_dim].copy(), U[:, ::-1][:, :state_dim].copy()
    for k in range(state_dim):
        if U[np.argmax(np.abs(U[:, k])), k] < 0:
            U[:, k] = -U[:, k]
    return lam, U


def _gram_hip(x, device, split):
    import torch
    from srlhip import _lib
    N, F = x.shape
    gram = torch.empty((N, N), dtype=torch.int64, device=device)
    rowsum = torch.empty((N,), dtype=torch.int64, device=device)
    _lib.pca_gram(device.index, x.data_ptr(), N, F, gram.data_ptr(), rowsum.data_ptr(), split=split,
                  stream=torch.cuda.current_stream(device).cuda_stream)
    colsum = x.sum(dim=0, dtype=torch.int64)
    return gram.cpu().numpy(), rowsum.cpu().numpy(), colsum.cpu().numpy()


def _project_hip(x, W, device):
    import torch
    from srlhip import _lib
    N, F = x.shape
    xt = x.t().contiguous()                                  # [F][N]: a device copy of the bytes
    out = torch.empty((F, W.shape[1]), dtype=torch.float64, device=device)
    proj = _lib.PcaProjector(device.index, W, np.zeros(W.shape[1]))
    try:
        proj.forward(xt.data_ptr(), F, out.data_ptr(), stream=torch.cuda.current_stream(device).cuda_stream)
        return out.cpu().numpy()
    finally:
        proj.close()


def fit_pca(frames, state_dim, backend="auto", device_id=None, split=0):
    """frames: uint8 [N][H][W][C] (any trailing shape), a device tensor or numpy -> FittedPCA.  backend "hip": the Gram matrix and the
    back-projection on the GPU (numpy frames are uploaded); "host": the library's host twins; "auto": hip where a GPU is visible."""
    import torch
    from srlhip import _lib
    if backend not in ("auto", "hip", "host"):
        raise ValueError("backend must be auto, hip or host")
    is_tensor = isinstance(frames, torch.Tensor)
    if backend == "auto":
        backend = "hip" if (frames.is_cuda if is_tensor else torch.cuda.is_available()) else "host"
    N = int(frames.shape[0])
    F = int(np.prod(tuple(frames.shape[1:]))) if frames.ndim > 1 else 0
    state_dim = int(state_dim)
    if not (frames.dtype == torch.uint8 if is_tensor else frames.dtype == np.uint8):
        raise ValueError("fit_pca takes uint8 frames (got {})".format(frames.dtype))
    if not _lib.pca_gram_supported(N, F):
        raise ValueError("fit_pca: {} frames of {} features (1..{} frames, 2 N^2 F 65025 < 2^63)".format(N, F, MAX_FRAMES))
    if not 1 <= state_dim <= min(MAX_DIM, N - 1):
        raise ValueError("fit_pca: state_dim must be 1..min({}, N - 1) (got {} for {} frames)".format(MAX_DIM, state_dim, N))
    if backend == "hip":
        if not torch.cuda.is_available():
            raise RuntimeError("fit_pca(backend='hip') needs a GPU")
        x = frames if is_tensor else torch.from_numpy(np.ascontiguousarray(frames))
        device = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device() if device_id is None else device_id)
        x = x.to(device).reshape(N, F).contiguous()
        gram, _, colsum = _gram_hip(x, device, split)
    else:
        x = np.ascontiguousarray(frames.cpu().numpy() if is_tensor else frames).reshape(N, F)
        gram, _ = _lib.pca_gram_host(x)
        colsum = x.sum(axis=0, dtype=np.int64)
    C = centred_gram(gram)
    lam, U = top_pairs(C, state_dim)
    if not (lam > 0).all():
        raise ValueError("fit_pca: the frames vary in fewer than {} directions (eigenvalues {})".format(state_dim, lam))
    mean = colsum.astype(np.float64) / np.float64(N)
    W = np.ascontiguousarray(U / np.sqrt(lam)[None, :])
    proj = _project_hip(x, W, device) if backend == "hip" else _lib.pca_project_host(W, np.zeros(state_dim), np.ascontiguousarray(x.T))
    comp = proj - mean[:, None] * W.sum(axis=0)[None, :]
    total = np.trace(C)
    return FittedPCA(np.ascontiguousarray(comp.T), mean, lam / (N - 1), np.sqrt(lam), lam / total, N, backend)


def collect_frames(env, n_steps, seed=0):
    """n_steps x num_envs frames of a RawPixelVecEnv under uniformly random actions drawn on the device: reset, then n_steps - 1 steps,
    each frame copied device to device -> uint8 tensor [n_steps num_envs][H][W][C], no host round trip"""
    import torch
    gen = torch.Generator(device=env.device).manual_seed(int(seed))
    out = torch.empty((n_steps,) + tuple(env.images.shape), dtype=torch.uint8, device=env.device)
    out[0].copy_(env.reset())
    for t in range(1, n_steps):
        if env.cfg.is_discrete:
            act = torch.randint(0, env.action_space.n, (env.num_envs,), device=env.device, generator=gen).to(torch.int32)
        else:
            act = torch.rand(tuple(env.actions.shape), device=env.device, generator=gen) * 2.0 - 1.0
        out[t].copy_(env.step(act)[0])
    return out.reshape((n_steps * env.num_envs,) + tuple(env.images.shape[1:]))


def fit_pca_from_env(env, n_steps, state_dim, seed=0):
    """a model fitted on the frames of a RawPixelVecEnv, collected and fitted on the env's device"""
    return fit_pca(collect_frames(env, n_steps, seed=seed), state_dim, backend="hip")


def load_dataset_frames(data_folder, max_frames=4096, backend="pillow", device_id=None):
    """the record_*/frame*.jpg of a dataset `dataset_generator` wrote, subsampled evenly down to max_frames -> uint8 [N][H][W][3].
    backend "pillow": decoded on the host, a numpy array; "hip": the files' bytes are uploaded and decoded on the GPU
    (srlhip.jpeg_io.decode_files: only streams of this library's encoder, `dataset_generator --device-jpeg`; ValueError names the first
    file that is not one), a device tensor; "auto": hip when a GPU is visible and every selected file is such a stream, else pillow;
    "hip-baseline": decoded on the GPU by srlhip_jpeg_decode_baseline, which also reads what the default recorder (Pillow) and the
    reference's (OpenCV) write — baseline JPEG, 4:2:0 or 4:4:4, standard Huffman tables; ValueError names the first file that is not
    one and says why."""
    if backend not in ("pillow", "hip", "auto", "hip-baseline"):
        raise ValueError("backend must be pillow, hip, auto or hip-baseline")
    paths = sorted(glob.glob(os.path.join(data_folder, "record_*", "frame*.jpg")))
    if not paths:
        raise ValueError("no record_*/frame*.jpg under {}".format(data_folder))
    max_frames = min(int(max_frames), MAX_FRAMES)
    if len(paths) > max_frames:
        paths = [paths[i] for i in np.linspace(0, len(paths) - 1, max_frames).round().astype(int)]
    if backend != "pillow":
        import torch
        from srlhip import jpeg_io
        if backend in ("hip", "hip-baseline") and not torch.cuda.is_available():
            raise RuntimeError("load_dataset_frames(backend='{}') needs a GPU".format(backend))
        if backend == "hip-baseline":
            return jpeg_io.decode_files(paths, torch.device("cuda", torch.cuda.current_device() if device_id is None else device_id), accept="baseline")
        if backend == "hip" or (torch.cuda.is_available() and jpeg_io.all_accepted(paths)):
            return jpeg_io.decode_files(paths, torch.device("cuda", torch.cuda.current_device() if device_id is None else device_id))
    from PIL import Image
    return np.stack([np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8) for p in paths])


def main(argv=None):
    parser = argparse.ArgumentParser(description="Fit the PCA state baseline on a recorded dataset")
    parser.add_argument("--data-folder", required=True, help="a dataset written by environments.dataset_generator")
    parser.add_argument("--state-dim", type=int, required=True)
    parser.add_argument("--max-frames", type=int, default=4096)
    parser.add_argument("--device-id", type=int, default=0)
    parser.add_argument("--backend", default="auto", choices=("auto", "hip", "host"))
    parser.add_argument("--decode-backend", default="pillow", choices=("pillow", "hip", "auto", "hip-baseline"),
                        help="who decodes the recorded JPEG files: Pillow on the host, or the GPU (hip: streams of --device-jpeg datasets only; "
                             "hip-baseline: also the default recorder's files)")
    parser.add_argument("--log-folder", required=True, help="the model goes to <log-folder>/baselines/pca_ST_DIM<k>/pca.pkl")
    parser.add_argument("--evaluate", action="store_true", default=False,
                        help="score the saved model on the frames it was fitted on (state_representation.evaluate: knn_mse.json next to the model)")
    args = parser.parse_args(argv)
    indices = None
    if args.evaluate:                    # the frames in ground_truth.npz's order, so that each keeps its ground-truth row
        from state_representation import evaluate
        paths, indices = evaluate.dataset_items(args.data_folder, min(int(args.max_frames), MAX_FRAMES))
        frames = evaluate.decode_items(paths, args.decode_backend, args.device_id)
    else:
        frames = load_dataset_frames(args.data_folder, args.max_frames, backend=args.decode_backend, device_id=args.device_id)
    model = fit_pca(frames, args.state_dim, backend=args.backend, device_id=args.device_id)
    path = model.save(args.log_folder)
    print("fitted {} components on {} frames of {} ({}): explained variance ratio {:.4f} -> {}".format(
        model.n_components_, len(frames), "x".join(str(d) for d in frames.shape[1:]), model.backend,
        float(model.explained_variance_ratio_.sum()), path))
    if args.evaluate:
        out = evaluate.evaluate_model(args.data_folder, path, backend=args.backend, device_id=args.device_id, log_folder=os.path.dirname(path),
                                      frames=frames, indices=indices)
        print("knn_mse {:.6g} (k = {}, {} queries; ground truth as states {:.6g}), gtc_mean {:.4f}".format(
            out["knn_mse"], out["k"], out["n_queries"], out["knn_mse_ground_truth"], out["gtc_mean"]))
    return path


if __name__ == "__main__":
    # (through the module's own name, so that the pickled FittedPCA names state_representation.pca_fit and not __main__)
    from state_representation.pca_fit import main as _main
    _main()
