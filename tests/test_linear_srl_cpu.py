"""srlhip_linear_srl_* and the linear SRL trainer without a GPU: the library's host twins (the kernels' own text, csrc/linear_srl.hpp)
against the numpy restatement bit for bit and against an exactly rounded reference within the derived bounds (tests/linear_srl_ref.py),
the Adam update against torch.optim.Adam, the stand-alone host program — plain and under the address / undefined-behaviour sanitizers —
against the library, the refusals, the trainer's "host" backend against its "torch" backend on a synthetic dataset, and the saved folder
through loadSRLModel."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import linear_srl_ref as ref

sys.path.insert(0, os.path.join(ref.REPO, "robotics-rl-srl_amd"))
from srlhip import _lib  # noqa: E402
from state_representation import linear_srl  # noqa: E402
from state_representation.models import SRLLinear, linear_from_checkpoint, linear_tables, linear_to_checkpoint, loadSRLModel  # noqa: E402

CASE_IDS = range(len(ref.CASES))


@pytest.fixture(scope="module")
def cases():
    """per case: the inputs, the host twin's states and its (grad, V, m, v) after one and after three steps — computed once"""
    out = []
    for shape, fill, grads in ref.CASES:
        case = ref.make_case(shape, fill, grads)
        states = _lib.linear_srl_forward_host(case["frames"], case["scale"], case["offset"], case["V"], case["c"])
        out.append((case, states, ref.host_steps(_lib, case, 1), ref.host_steps(_lib, case, 3)))
    return out


@pytest.fixture(scope="module")
def programs():
    ref.build_programs()
    return ref.PROGRAMS


@pytest.mark.parametrize("k", CASE_IDS, ids=ref.IDS)
def test_host_twins_equal_the_numpy_restatement_bit_for_bit(cases, k):
    case, states, one, three = cases[k]
    assert ref.same_bits(states, ref.forward(case["frames"], case["scale"], case["offset"], case["V"], case["c"]))
    g = ref.gradient(case["frames"], case["scale"], case["offset"], case["G"])
    assert ref.same_bits(one[0], g) and ref.same_bits(three[0], g)
    V, m, v = case["V"], np.zeros_like(g), np.zeros_like(g)
    for t in range(3):
        V, m, v = ref.adam_step(g, V, m, v, ref.adam_at(t + 1))
        if t == 0:
            assert ref.same_bits(one[1], V) and ref.same_bits(one[2], m) and ref.same_bits(one[3], v)
    assert ref.same_bits(three[1], V) and ref.same_bits(three[2], m) and ref.same_bits(three[3], v)


@pytest.mark.parametrize("k", CASE_IDS, ids=ref.IDS)
def test_host_twins_within_the_derived_bounds_of_the_exact_reference(cases, k):
    case, states, one, _ = cases[k]
    F, S = case["V"].shape
    n = len(case["frames"])
    want, T = ref.exact_forward(case["frames"], case["scale"], case["offset"], case["V"], case["c"])
    err, bnd = np.abs(states - want), ref.forward_bound(F, T)
    print("forward: max |twin - exact| / bound", float((err / np.maximum(bnd, 1e-300)).max()))
    assert (err <= bnd).all() and (T > 0).all()
    rows = np.unique(np.linspace(0, F - 1, 40).round().astype(int))          # (the exact sum is slow: 40 feature rows, first and last among them)
    want, T = ref.exact_gradient(case["frames"], case["scale"], case["offset"], case["G"], rows)
    err, bnd = np.abs(one[0][rows] - want), ref.gradient_bound(n, T)
    print("gradient: max |twin - exact| / bound", float((err / np.maximum(bnd, 1e-300)).max()))
    assert (err <= bnd).all() and np.isfinite(want).all()


def test_adam_against_torch_optim_adam():
    """Three steps from the same g.  torch's documented single-tensor order (torch/optim/adam.py): exp_avg.lerp_(grad, 1 - beta1) =
    m + (1 - beta1) (g - m); exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2); denom = (sqrt(v) / sqrt(bc2)).add_(eps);
    param.addcdiv_(exp_avg, denom, value=-(lr / bc1)).  It differs from the contract's in how m is formed (lerp: 3 roundings, ours: 3) and
    in where the step size is multiplied in; each form rounds m, v, sqrt, the two quotients, the sum and the product once or twice, a
    relative error of the UPDATE of at most ~12 x 2^-53 per form and step.  The update is at most lr / bc1 x |m| / (sqrt(v) / sqrt(bc2))
    <= ~lr x 3.2 in magnitude (|m_hat| / sqrt(v_hat) <= 1 / sqrt(1 - beta2) at worst, ~1 for a constant g), so after three steps
    |V - V_torch| <= 3 x 2 x 12 x 2^-53 x lr x 3.2 + 3 x 2^-53 |V| (the subtraction's own rounding): TOL below.  Measured maximum of
    |V - V_torch| / TOL on these cases: 0.48 (a few ulps of V)."""
    lr = 1e-3
    worst = 0.0
    for shape in ((193, 5, 3, 3), (130, 40, 3, 6)):
        case = ref.make_case(shape)
        g, V, _, _ = ref.host_steps(_lib, case, 3)
        p = torch.nn.Parameter(torch.from_numpy(case["V"].copy()))
        opt = torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999), eps=1e-8)
        for _ in range(3):
            p.grad = torch.from_numpy(g.copy())
            opt.step()
        tol = 3 * 2 * 12 * 2.0 ** -53 * lr * 3.2 + 3 * 2.0 ** -53 * np.abs(V)
        ratio = np.abs(V - p.detach().numpy()) / tol
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all()
        assert np.abs(V - case["V"]).max() > 0.5 * lr                     # (the steps moved V: about lr each)
    print("max |V - V_torch| / tolerance", worst)


@pytest.mark.parametrize("k", [0, 3, 4, 7, 11], ids=[ref.IDS[k] for k in (0, 3, 4, 7, 11)])
def test_host_programs_give_the_library_bits(programs, cases, tmp_path, k):
    case, states, one, three = cases[k]
    for program in programs:                               # the second one is the sanitised build: it must run clean and give the same bits
        for steps, want in ((1, one), (3, three)):
            got = ref.run_program(program, tmp_path, case, steps)
            assert ref.same_bits(got[0], states)
            for a, b in zip(got[1:], want):
                assert ref.same_bits(a, b)


def test_host_programs_check_and_rules(programs):
    for program in programs:
        exe = os.path.join(ref.CSRC, "build", program)
        assert subprocess.check_output([exe, "check"]).decode().strip() == "check ok"
        lines = subprocess.check_output([exe, "rules"]).decode().splitlines()
        shape = {tuple(int(v) for v in ln.split(":")[0].split()[1:]): ln.split(": ", 1)[1] for ln in lines if ln.startswith("shape ")}
        assert len(shape) == 48
        for (F, S, C), verdict in shape.items():
            ok = F >= 1 and 1 <= S <= ref.MAX_DIM and 1 <= C <= ref.MAX_CHANNELS
            assert verdict == "0 accepted" if ok else verdict.startswith("-95 linear_srl: "), (F, S, C, verdict)
            assert _lib.linear_srl_supported(F, S, C) == ok
        assert [ln.split(": ", 1)[1].split(" ")[0] for ln in lines if ln.startswith("batch ")] == ["-22", "-22", "0", "0", "-95"]
        assert [ln.split(": ", 1)[1].split(" ")[0] for ln in lines if ln.startswith("tables ")] == ["0", "-22", "-22"]
        assert [ln.split(": ", 1)[1].split(" ")[0] for ln in lines if ln.startswith("adam ")] == ["0"] + ["-22"] * 6
        for ln in (ln for ln in lines if ln.startswith("launch ")):
            t = ln.replace(":", "").split()
            F, S, n, nc, SP, tiles, work, group, groups, blocks = (int(t[i]) for i in (2, 4, 6, 8, 10, 12, 14, 16, 18, 20))
            assert nc == ref.chunks(F) and SP >= S and SP in (8, 16, 32, 64) and SP < 2 * max(S, 5)
            assert work == nc * n * SP * 8 == _lib.linear_srl_workspace_bytes(F, S, n)
            assert group in (8, 16, 32) and groups == -(-S // group) and groups * group < S + group and blocks == -(-F // 128)
            assert tiles == -(-n // (2 * 256 // (SP // 8)))


def test_refusals_leave_sentinelled_buffers_untouched():
    lib = _lib.load()
    case = ref.make_case((193, 5, 2, 3))
    F, S = case["V"].shape
    sentinel = -1234.5
    V, m, v, g, states = (np.full(shape, sentinel) for shape in ((F, S), (F, S), (F, S), (F, S), (2, S)))
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    dbl = ctypes.c_double
    good = [dbl(x) for x in (1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001)]

    def fwd(n=2, F_=F, S_=S, C=3, scale=case["scale"], offset=case["offset"], frames=case["frames"], out=states):
        return lib.srlhip_linear_srl_forward_host(ptr(frames), n, F_, S_, C, ptr(scale), ptr(offset), ptr(V), ptr(case["c"]), ptr(out))

    def step(n=2, S_=S, C=3, adam=good, G=case["G"], scale=case["scale"], mm=m):
        return lib.srlhip_linear_srl_step_host(ptr(case["frames"]), n, F, S_, C, ptr(scale), ptr(case["offset"]), ptr(G), ptr(V), ptr(mm), ptr(v),
                                               *(adam + [ptr(g)]))

    def with_(i, x):
        return good[:i] + [dbl(x)] + good[i + 1:]

    inf3 = np.array([1.0, np.inf, 1.0])
    assert fwd(n=0) == -22 and fwd(n=-3) == -22 and fwd(n=1025) == -95 and fwd(S_=0) == -95 and fwd(S_=65) == -95 and fwd(F_=0) == -95
    assert fwd(C=0) == -95 and fwd(C=9) == -95 and fwd(scale=None) == -22 and fwd(offset=inf3) == -22 and fwd(frames=None) == -22
    assert fwd(out=None) == -22
    assert b"linear_srl" in lib.srlhip_linear_srl_last_error()
    assert step(n=0) == -22 and step(n=1025) == -95 and step(S_=65) == -95 and step(C=9) == -95 and step(G=None) == -22 and step(mm=None) == -22
    assert step(scale=inf3) == -22
    for i, x in ((0, float("nan")), (0, float("inf")), (1, 1.0), (1, -0.1), (2, 1.0), (3, -1e-8), (3, float("nan")), (4, 0.0), (4, 1.5), (5, 0.0)):
        assert step(adam=with_(i, x)) == -22, (i, x)
    assert b"srlhip_linear_srl_step_host: linear_srl: bc1 and bc2" in lib.srlhip_linear_srl_last_error()
    for a in (V, m, v, g, states):
        assert (a == sentinel).all()
    # the device calls refuse the same arguments before they touch the GPU (none is needed for this): null device pointers stand in
    assert lib.srlhip_linear_srl_forward(0, None, 1025, F, S, 3, ptr(case["scale"]), ptr(case["offset"]), None, None, None, None, None) == -95
    assert lib.srlhip_linear_srl_step(0, None, 2, F, S, 3, ptr(case["scale"]), ptr(case["offset"]), None, None, None, None, *(good + [None, None])) == -22
    assert _lib.linear_srl_workspace_bytes(F, 65, 2) == 0 and _lib.linear_srl_workspace_bytes(F, S, 1025) == 0
    with pytest.raises(_lib.SrlHipError):
        _lib.linear_srl_forward_host(case["frames"], np.ones(9), np.ones(9), case["V"], case["c"])


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------
H, W, EPISODES, LENGTH = 8, 8, 3, 20


@pytest.fixture(scope="module")
def dataset():
    """8 x 8 x 3 frames, 3 episodes of 20 steps; the ground truth is a linear function of the normalised pixels (plus a constant)"""
    rng = np.random.RandomState(5)
    N = EPISODES * LENGTH
    frames = rng.randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)
    scale, offset = linear_tables(3)
    xn = frames.reshape(N, -1) * np.tile(scale, H * W) - np.tile(offset, H * W)
    truth = xn @ (rng.standard_normal((H * W * 3, 2)) / np.sqrt(H * W * 3)) + np.array([0.3, -0.2])
    starts = np.zeros(N, bool)
    starts[::LENGTH] = True
    return frames, rng.randint(0, 4, size=N), starts, truth


def _fit(dataset, backend, losses, state_dim, epochs, lr=1e-2):
    frames, actions, starts, truth = dataset
    trainer = linear_srl.LinearSRLTrainer((H, W), 3, state_dim, losses, 4, backend=backend, learning_rate=lr, seed=1)
    return trainer, trainer.fit(frames, actions, starts, truth, epochs=epochs, batch_size=16, seed=2)


def test_trainer_host_backend_against_the_torch_backend(dataset):
    """supervised, 30 epochs of 4 batches = 120 steps at lr = 1e-2.  The torch backend alone, measured once: the epoch-mean loss falls from
    2.788 (epoch 0) to 3.80e-5 (epoch 29), a factor of 7.3e4; the test asks for half of that factor, 3.6e4, of both backends.
    The two backends run the same algorithm in different float64 operation orders (BLAS against the contract's chunks, lerp against the
    contract's Adam): a step's update differs by a relative ~1e-13 at most (a few hundred roundings of 2^-53 on sums of 192 terms, and
    Adam's normalisation m / sqrt(v) passes relative errors of g on undamped), i.e. lr x 1e-13 = 1e-15 absolute per step, but the
    difference also feeds back through the next gradients; with |V| growth bounded by lr per step the recursion stays linear over 120
    steps: 120 x 1e-15 x a feedback factor of 10 gives ~1e-12.  The tolerance is 1e-10 absolute on entries of magnitude ~0.1; the
    measured maximum difference is printed (1.9e-16 when this was written)."""
    host, h_hist = _fit(dataset, "host", ["supervised"], 2, 30)
    ref_, t_hist = _fit(dataset, "torch", ["supervised"], 2, 30)
    print("torch epoch losses", t_hist[0], t_hist[-1], "host", h_hist[0], h_hist[-1])
    assert t_hist[-1] * 3.6e4 < t_hist[0] and h_hist[-1] * 3.6e4 < h_hist[0]
    (Vh, ch), (Vt, ct) = host.encoder.weights(), ref_.encoder.weights()
    print("max |V host - V torch|", np.abs(Vh - Vt).max(), "max |c host - c torch|", np.abs(ch - ct).max())
    assert np.abs(Vh - Vt).max() < 1e-10 and np.abs(ch - ct).max() < 1e-10
    assert host.encoder.t == 120


def test_trainer_pair_losses_drop_the_episode_seams(dataset):
    frames, actions, starts, truth = dataset
    host, h_hist = _fit(dataset, "host", ["inverse", "forward"], 3, 2)
    ref_, t_hist = _fit(dataset, "torch", ["inverse", "forward"], 3, 2)
    # 57 pairs = 3 x 19 -> 4 batches of at most 16 per epoch
    assert host.encoder.t == 8 and np.isfinite(h_hist).all()
    assert np.allclose(h_hist, t_hist, rtol=1e-9) and np.abs(host.encoder.weights()[0] - ref_.encoder.weights()[0]).max() < 1e-10
    with pytest.raises(ValueError):
        host.fit(frames, actions, starts, truth, batch_size=513)              # 1026 frames per call
    with pytest.raises(ValueError):
        linear_srl.LinearSRLTrainer((H, W), 3, 3, ["inverse", "reward"], 4, backend="host")


@pytest.mark.parametrize("losses", [["supervised"], ["inverse", "forward"]], ids=["supervised", "inverse forward"])
def test_saved_folder_round_trips_through_load_srl_model(dataset, tmp_path, losses):
    frames = dataset[0]
    trainer, _ = _fit(dataset, "host", losses, 2, 1)
    path = trainer.save(str(tmp_path))
    folder = os.path.dirname(path)
    if losses == ["supervised"]:
        assert path == os.path.join(str(tmp_path), "baselines", "supervised_linear_ST_DIM2", "srl_supervised_model.pth")
        assert sorted(torch.load(path)) == ["fc.bias", "fc.weight"]
    else:
        assert path == os.path.join(str(tmp_path), "srl_model.pth")
        sd = torch.load(path)
        assert sorted(sd) == ["forward_net.bias", "forward_net.weight", "inverse_net.bias", "inverse_net.weight", "model.fc.bias", "model.fc.weight"]
        assert tuple(sd["inverse_net.weight"].shape) == (4, 4) and tuple(sd["forward_net.weight"].shape) == (2, 6)
        assert tuple(sd["model.fc.weight"].shape) == (2, H * W * 3) and sd["model.fc.weight"].dtype == torch.float64
    with open(os.path.join(folder, "exp_config.json")) as f:
        cfg = json.load(f)
    assert cfg["state-dim"] == 2 and cfg["losses"] == losses and cfg["n_actions"] == 4 and cfg["model-type"] == "linear"
    assert cfg["inverse-model-type"] == "linear" and cfg["split-dimensions"] == -1
    model = loadSRLModel(path, cuda=False, img_shape=(H, W), n_channels=3)
    assert isinstance(model, SRLLinear) and model.state_dim == 2 and model.state_dtype == torch.float64 and model.hip is None
    assert model.losses == losses and model.n_actions == 4 and model.split_dimensions is None
    got = model.getStates(frames).numpy()
    want = trainer.encoder.forward(frames).numpy()
    # the fold: states = x (scale V) + (c - offset^T V) on the raw bytes against sum (scale x - offset) V + c.  Both sum F + 1 terms of
    # magnitude |x scale V|, |offset V| and |c| with at most F + 3 roundings each: (F + 3) 2^-52 T bounds their difference
    V, c = trainer.encoder.weights()
    scale, offset = linear_tables(3)
    x = frames.reshape(len(frames), -1).astype(np.float64)
    T = (x * np.tile(scale, H * W)) @ np.abs(V) + (np.tile(offset, H * W)[:, None] * np.abs(V)).sum(axis=0) + np.abs(c)
    print("max |getStates - forward| / bound", float((np.abs(got - want) / ((H * W * 3 + 3) * 2.0 ** -52 * T)).max()))
    assert (np.abs(got - want) <= (H * W * 3 + 3) * 2.0 ** -52 * T).all()
    assert np.allclose(model.getState(frames[0]), got[0], rtol=1e-12, atol=1e-12)
    twin = model.replicate("cpu")
    assert isinstance(twin, SRLLinear) and np.array_equal(twin.getStates(frames).numpy(), got) and twin.losses == losses


def test_flatten_permutation_on_a_non_square_frame():
    """The reference's network sees preprocess(frame) = [C][W][H] (width and height swapped) flattened: fc.weight's column f' belongs to
    pixel (h, w, ch) with f' = (ch W + w) H + h.  Checked against torch's own preprocess + nn.Linear on a 4 x 6 x 3 frame."""
    from state_representation.models import preprocess
    Hn, Wn, C, S = 4, 6, 3, 2
    rng = np.random.RandomState(9)
    fc = torch.nn.Linear(Hn * Wn * C, S).double()
    frames = rng.randint(0, 256, size=(5, Hn, Wn, C)).astype(np.uint8)
    with torch.no_grad():
        want = fc(preprocess(torch.from_numpy(frames)).to(torch.float64).reshape(5, -1)).numpy()
    model = SRLLinear(S, cuda=False, img_shape=(Hn, Wn), n_channels=C)
    sd = {"fc." + k: v for k, v in fc.state_dict().items()}
    model.set_model(sd)
    assert np.allclose(model.getStates(frames).numpy(), want, rtol=0, atol=1e-6)          # (preprocess is float32: 2^-24 relative per pixel)
    V = linear_from_checkpoint(fc.weight.detach().numpy(), (Hn, Wn), C)
    h, w, ch = 3, 4, 1
    assert np.array_equal(V[(h * Wn + w) * C + ch], fc.weight.detach().numpy()[:, (ch * Wn + w) * Hn + h])
    assert np.array_equal(linear_to_checkpoint(V, (Hn, Wn), C), fc.weight.detach().numpy())
    with pytest.raises(ValueError):
        SRLLinear(S, cuda=False, img_shape=(Hn, Wn + 1), n_channels=C).set_model(sd)
    with pytest.raises(KeyError):
        model.set_model({"fc.weight": fc.weight, "fc.bias": fc.bias, "conv.weight": fc.bias})
