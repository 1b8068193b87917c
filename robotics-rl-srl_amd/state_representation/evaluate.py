"""Score a state representation: exact k nearest neighbours in the learned state space and KNN-MSE, the number the reference computes
after every SRL training (its tests/test_end_to_end.py passes `knn-samples` / `knn-seed` and reads the `NearestNeighbors/` folder; the
code itself lives in srl_zoo, an empty submodule of the reference checkout).

For sampled frames, find the k nearest neighbours in state space and average the squared distance of their ground-truth states to the
frame's own: a representation in which neighbouring states are neighbouring robot positions scores low.  The neighbour search is
srlhip_knn (csrc/knn.hip; the contract is in include/srlhip.h) on the GPU or its host twin: exact float64 distances in a fixed order and
a total order of the candidates, so both backends — and every split of the work — give the same bits.

    python -m state_representation.evaluate --data-folder D --srl-model-path P [--state-dim K] [--k 5] [--knn-samples Q] [--knn-seed 1]
        [--max-frames 4096] [--decode-backend pillow|hip|auto|hip-baseline] [--backend auto|hip|host] [--device-id 0] [--log-folder OUT]
"""
import argparse
import json
import os

import numpy as np


def _resolve_backend(backend, tensors):
    import torch
    if backend not in ("auto", "hip", "host"):
        raise ValueError("backend must be auto, hip or host")
    if backend == "auto":
        on_device = [t.is_cuda for t in tensors if isinstance(t, torch.Tensor)]
        backend = "hip" if (any(on_device) if on_device else torch.cuda.is_available()) else "host"
    if backend == "hip" and not torch.cuda.is_available():
        raise RuntimeError("backend='hip' needs a GPU")
    return backend


def _to_numpy(a):
    import torch
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def nearest_neighbours(states, k, queries=None, ground_truth=None, backend="auto", split=0, device_id=None):
    """states [N][S] float64 or float32 (anything else is converted to float64), a torch tensor or numpy; queries int [Q] row indices or
    None (every row); ground_truth [N][G] or None -> (idx int32 [Q][k], dist float64 [Q][k][, err float64 [Q]]) as numpy arrays.
    backend "hip": srlhip_knn on the GPU (numpy inputs are uploaded); "host": the library's host twin; "auto": hip where the states are
    on a GPU, or, for numpy, where one is visible.  Non-finite states are refused here (ValueError): the library itself only keeps a NaN
    distance out of every list."""
    import torch
    from srlhip import _lib
    backend = _resolve_backend(backend, (states, ground_truth))
    if states.ndim != 2:
        raise ValueError("nearest_neighbours takes states [N][S]")
    N, S = int(states.shape[0]), int(states.shape[1])
    G = 0 if ground_truth is None else int(ground_truth.shape[1])
    if ground_truth is not None and (ground_truth.ndim != 2 or int(ground_truth.shape[0]) != N):
        raise ValueError("nearest_neighbours takes ground_truth [N][G]")
    if queries is not None:
        queries = np.ascontiguousarray(_to_numpy(queries), dtype=np.int64).reshape(-1)
        if len(queries) and (queries.min() < 0 or queries.max() >= N):
            raise ValueError("nearest_neighbours: a query index is outside 0..{}".format(N - 1))
        queries = queries.astype(np.int32)
    Q = N if queries is None else len(queries)
    k = int(k)
    if not _lib.knn_supported(N, S, k, Q, G):
        raise ValueError("nearest_neighbours: {} states of {} dimensions, k = {}, {} queries, {} ground-truth dimensions (2 <= N <= 2^20, "
                         "S <= 64, 1 <= k <= min(32, N - 1), 1 <= Q <= 2^20, G <= 32)".format(N, S, k, Q, G))
    if backend == "host":
        x = _to_numpy(states)
        x = np.ascontiguousarray(x, dtype=np.float32 if x.dtype == np.float32 else np.float64)
        gt = None if ground_truth is None else np.ascontiguousarray(_to_numpy(ground_truth), dtype=np.float64)
        if not np.isfinite(x).all() or (gt is not None and not np.isfinite(gt).all()):
            raise ValueError("nearest_neighbours: non-finite states or ground truth")
        return _lib.knn_host(x, k, queries, gt)
    x = states if isinstance(states, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(states))
    device = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device() if device_id is None else device_id)
    x = x.to(device)
    x = (x if x.dtype in (torch.float32, torch.float64) else x.to(torch.float64)).contiguous()
    gt = None
    if ground_truth is not None:
        gt = ground_truth if isinstance(ground_truth, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ground_truth))
        gt = gt.to(device).to(torch.float64).contiguous()
    if not bool(torch.isfinite(x).all()) or (gt is not None and not bool(torch.isfinite(gt).all())):
        raise ValueError("nearest_neighbours: non-finite states or ground truth")
    qd = None if queries is None else torch.from_numpy(queries).to(device)
    idx = torch.empty((Q, k), dtype=torch.int32, device=device)
    dist = torch.empty((Q, k), dtype=torch.float64, device=device)
    err = torch.empty((Q,), dtype=torch.float64, device=device) if gt is not None else None
    work = torch.empty((_lib.knn_workspace_bytes(N, S, k, Q, split) + 7) // 8, dtype=torch.int64, device=device)
    _lib.knn(device.index, x.data_ptr(), x.dtype == torch.float32, N, S, None if qd is None else qd.data_ptr(), Q, k,
             None if gt is None else gt.data_ptr(), G, idx.data_ptr(), dist.data_ptr(), None if err is None else err.data_ptr(),
             work.data_ptr(), split=split, stream=torch.cuda.current_stream(device).cuda_stream)
    out = (idx.cpu().numpy(), dist.cpu().numpy())           # (the copies wait for the stream)
    return out if err is None else out + (err.cpu().numpy(),)


def sample_queries(n, n_samples=None, seed=1):
    """None: every frame; otherwise np.sort(np.random.RandomState(seed).choice(n, n_samples, replace=False))"""
    if n_samples is None or int(n_samples) >= n:
        return None
    return np.sort(np.random.RandomState(seed).choice(n, int(n_samples), replace=False)).astype(np.int32)


def knn_mse(states, ground_truth, k=5, n_samples=None, seed=1, backend="auto", split=0, device_id=None):
    """-> dict(knn_mse, k, n_queries, n_frames, backend, queries, idx, dist, err).  knn_mse = float(np.mean(err)), err[q] the mean over the
    k nearest neighbours (in state space) of query q of the squared Euclidean distance between their ground-truth states and the query's
    (srlhip_knn's err).  n_samples=None: every frame is a query; otherwise the queries are sample_queries(N, n_samples, seed).  The same
    numpy line finishes both backends, so both give the same bits.
    The function that produces the reference's end-of-training number is srl_zoo's and cannot be read in the reference checkout: the
    default k = 5 and this definition of KNN-MSE are recalled from the toolbox's paper, not checked against that code."""
    N = int(states.shape[0])
    queries = sample_queries(N, n_samples, seed)
    backend = _resolve_backend(backend, (states, ground_truth))
    idx, dist, err = nearest_neighbours(states, k, queries, ground_truth, backend=backend, split=split, device_id=device_id)
    return {"knn_mse": float(np.mean(err)), "k": int(k), "n_queries": int(len(err)), "n_frames": N, "backend": backend,
            "queries": np.arange(N, dtype=np.int32) if queries is None else queries, "idx": idx, "dist": dist, "err": err}


def ground_truth_correlation(states, ground_truth):
    """-> (gtc float64 [G], gtc_mean): gtc[g] = max_s |corr(state_s, gt_g)| with numpy's float64 corrcoef on the host; a constant column
    (whose correlation is undefined) counts as 0, not NaN"""
    x = np.asarray(_to_numpy(states), dtype=np.float64)
    gt = np.asarray(_to_numpy(ground_truth), dtype=np.float64)
    S = x.shape[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.corrcoef(x, gt, rowvar=False)[:S, S:]
    c = np.where(np.isfinite(c), np.abs(c), 0.0)
    gtc = c.max(axis=0)
    return gtc, float(gtc.mean())


def dataset_items(data_folder, max_frames=4096):
    """-> (paths, indices): the JPEG files of a recorded dataset in the order of ground_truth.npz's `images_path` and their row numbers
    there, subsampled evenly down to max_frames with load_dataset_frames' np.linspace rule, so that the frames and
    ground_truth_states[indices] stay paired"""
    with np.load(os.path.join(data_folder, "ground_truth.npz"), allow_pickle=True) as gt:
        names = [str(p) for p in gt["images_path"]]
    indices = np.arange(len(names))
    if len(names) > int(max_frames):
        indices = np.linspace(0, len(names) - 1, int(max_frames)).round().astype(int)
    paths = [os.path.join(data_folder, *names[i].split("/")[1:]) + ".jpg" for i in indices]
    return paths, indices


def decode_items(paths, backend="pillow", device_id=0):
    """the files of dataset_items -> uint8 [N][H][W][3], numpy (pillow) or a device tensor (the GPU decoders of load_dataset_frames)"""
    if backend not in ("pillow", "hip", "auto", "hip-baseline"):
        raise ValueError("decode backend must be pillow, hip, auto or hip-baseline")
    if backend != "pillow":
        import torch
        from srlhip import jpeg_io
        if backend in ("hip", "hip-baseline") and not torch.cuda.is_available():
            raise RuntimeError("--decode-backend {} needs a GPU".format(backend))
        device = torch.device("cuda", device_id) if torch.cuda.is_available() else None
        if backend == "hip-baseline":
            return jpeg_io.decode_files(paths, device, accept="baseline")
        if backend == "hip" or (device is not None and jpeg_io.all_accepted(paths)):
            return jpeg_io.decode_files(paths, device)
    from PIL import Image
    return np.stack([np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8) for p in paths])


def model_states(model, frames, batch=256):
    """getStates over the frames in batches -> [N][state_dim] on the model's device (float32 for the encoder, float64 for the PCA)"""
    import torch
    out = []
    with torch.no_grad():
        for b in range(0, len(frames), batch):
            out.append(model.getStates(frames[b:b + batch]).clone())
    return torch.cat(out)


def evaluate_model(data_folder, model_path, state_dim=None, k=5, knn_samples=None, knn_seed=1, max_frames=4096, decode_backend="pillow",
                   backend="auto", device_id=0, log_folder=None, frames=None, indices=None):
    """Decode the dataset's frames (or take `frames` with their `indices` into ground_truth.npz), load the model with loadSRLModel, get
    the states in batches on the device, and score them -> the dict written to <log_folder>/knn_mse.json (with log_folder, also
    nearest_neighbours.npz: queries, idx, dist and the images_path of the selected frames)."""
    import torch
    from state_representation.models import loadSRLModel
    with np.load(os.path.join(data_folder, "ground_truth.npz"), allow_pickle=True) as f:
        gt_all, names = np.asarray(f["ground_truth_states"], dtype=np.float64), np.asarray([str(p) for p in f["images_path"]])
    if frames is None:
        paths, indices = dataset_items(data_folder, max_frames)
        frames = decode_items(paths, decode_backend, device_id)
    gt = gt_all[np.asarray(indices)].reshape(len(indices), -1)
    cuda = torch.cuda.is_available() and backend != "host"
    model = loadSRLModel(model_path, cuda=cuda, state_dim=state_dim, img_shape=tuple(frames.shape[1:3]), n_channels=int(frames.shape[3]),
                         device=torch.device("cuda", device_id) if cuda else None)
    states = model_states(model, frames)
    res = knn_mse(states, gt, k=k, n_samples=knn_samples, seed=knn_seed, backend=backend, device_id=device_id)
    floor = knn_mse(gt, gt, k=k, n_samples=knn_samples, seed=knn_seed, backend=res["backend"], device_id=device_id)
    gtc, gtc_mean = ground_truth_correlation(states, gt)
    out = {"knn_mse": res["knn_mse"], "k": res["k"], "n_queries": res["n_queries"], "n_frames": res["n_frames"], "gtc": [float(v) for v in gtc],
           "gtc_mean": gtc_mean, "srl_model_path": model_path, "backend": res["backend"], "knn_mse_ground_truth": floor["knn_mse"]}
    if log_folder is not None:
        os.makedirs(log_folder, exist_ok=True)
        with open(os.path.join(log_folder, "knn_mse.json"), "w") as f:
            json.dump(out, f, indent=2)
        np.savez(os.path.join(log_folder, "nearest_neighbours.npz"), queries=res["queries"], idx=res["idx"], dist=res["dist"],
                 images_path=names[np.asarray(indices)])
    return out


def main(argv=None):
    parser = argparse.ArgumentParser(description="KNN-MSE and ground-truth correlation of a state representation on a recorded dataset")
    parser.add_argument("--data-folder", required=True, help="a dataset written by environments.dataset_generator")
    parser.add_argument("--srl-model-path", required=True, help="what loadSRLModel takes: .../baselines/pca_ST_DIM<k>/pca.pkl or a srl_model.pth")
    parser.add_argument("--state-dim", type=int, default=None)
    parser.add_argument("--k", type=int, default=5)
    parser.add_argument("--knn-samples", type=int, default=None, help="number of query frames (default: every frame)")
    parser.add_argument("--knn-seed", type=int, default=1)
    parser.add_argument("--max-frames", type=int, default=4096)
    parser.add_argument("--decode-backend", default="pillow", choices=("pillow", "hip", "auto", "hip-baseline"))
    parser.add_argument("--backend", default="auto", choices=("auto", "hip", "host"))
    parser.add_argument("--device-id", type=int, default=0)
    parser.add_argument("--log-folder", default=None, help="knn_mse.json and nearest_neighbours.npz go here (default: next to the model)")
    args = parser.parse_args(argv)
    log_folder = args.log_folder if args.log_folder is not None else os.path.dirname(os.path.abspath(args.srl_model_path))
    out = evaluate_model(args.data_folder, args.srl_model_path, state_dim=args.state_dim, k=args.k, knn_samples=args.knn_samples,
                         knn_seed=args.knn_seed, max_frames=args.max_frames, decode_backend=args.decode_backend, backend=args.backend,
                         device_id=args.device_id, log_folder=log_folder)
    print("knn_mse {:.6g} (k = {}, {} queries of {} frames, {}; ground truth as states {:.6g}), gtc_mean {:.4f} -> {}".format(
        out["knn_mse"], out["k"], out["n_queries"], out["n_frames"], out["backend"], out["knn_mse_ground_truth"], out["gtc_mean"],
        os.path.join(log_folder, "knn_mse.json")))
    return out


if __name__ == "__main__":
    main()
