"""GPU: srlhip_linear_srl_forward / srlhip_linear_srl_step (csrc/linear_srl.hip) against the library's host twins BIT FOR BIT — the same
header functions (csrc/linear_srl.hpp), so the kernels hold tests/test_linear_srl_cpu.py's derived bounds transitively — with sentinels
around every written buffer, on a non-default stream, twice; and the trainer end to end: record, train, save, load, evaluate, roll out."""
import numpy as np
import pytest
import torch

import linear_srl_ref as ref
from srlhip import _lib

pytestmark = pytest.mark.gpu

PAD = 64                       # sentinel doubles in front of and behind every written buffer
SENTINEL = -1234.5


class Guarded(object):
    """a device float64 buffer between two runs of sentinels"""

    def __init__(self, shape, init=None):
        self.shape = tuple(shape)
        self.size = int(np.prod(self.shape))
        self.buf = torch.full((self.size + 2 * PAD,), SENTINEL, dtype=torch.float64, device="cuda")
        if init is not None:
            self.buf[PAD:PAD + self.size].copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float64).reshape(-1)))

    def ptr(self):
        return self.buf.data_ptr() + 8 * PAD

    def get(self):
        host = self.buf.cpu().numpy()
        assert (host[:PAD] == SENTINEL).all() and (host[PAD + self.size:] == SENTINEL).all(), "a sentinel was overwritten"
        return host[PAD:PAD + self.size].reshape(self.shape).copy()


def _device_run(case, steps, stream=None, n=None):
    """forward, then `steps` Adam steps with the case's G from m = v = 0 -> (states, grad of the last step, V, m, v)"""
    frames = case["frames"] if n is None else case["frames"][:n]
    G = case["G"] if n is None else case["G"][:n]
    n = len(frames)
    F, S = case["V"].shape
    raw = 0 if stream is None else stream.cuda_stream
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        x = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        Gd = torch.from_numpy(np.ascontiguousarray(G)).cuda()
        cd = torch.from_numpy(case["c"]).cuda()
        V, m, v, g = Guarded((F, S), case["V"]), Guarded((F, S), np.zeros((F, S))), Guarded((F, S), np.zeros((F, S))), Guarded((F, S))
        states = Guarded((n, S))
        nbytes = _lib.linear_srl_workspace_bytes(F, S, n)
        assert nbytes > 0
        work = Guarded((nbytes // 8,))
        torch.cuda.synchronize()
        _lib.linear_srl_forward(0, x.data_ptr(), n, F, S, case["scale"], case["offset"], V.ptr(), cd.data_ptr(), states.ptr(), work.ptr(), stream=raw)
        for t in range(steps):
            _lib.linear_srl_step(0, x.data_ptr(), n, F, S, case["scale"], case["offset"], Gd.data_ptr(), V.ptr(), m.ptr(), v.ptr(),
                                 ref.adam_at(t + 1), grad_out_ptr=g.ptr(), stream=raw)
        torch.cuda.synchronize()
    work.get()
    return states.get(), g.get(), V.get(), m.get(), v.get()


def _host_run(case, steps, n=None):
    sub = dict(case) if n is None else dict(case, frames=case["frames"][:n], G=case["G"][:n])
    states = _lib.linear_srl_forward_host(sub["frames"], sub["scale"], sub["offset"], sub["V"], sub["c"])
    return (states,) + ref.host_steps(_lib, sub, steps)


def _assert_same(got, want, what):
    for name, a, b in zip(("states", "grad", "V", "m", "v"), got, want):
        assert ref.same_bits(a, b), (what, name)


@pytest.mark.parametrize("case_id", range(len(ref.CASES)), ids=ref.IDS)
def test_kernels_equal_the_host_twins_bit_for_bit(case_id):
    shape, fill, grads = ref.CASES[case_id]
    case = ref.make_case(shape, fill, grads)
    for steps in (1, 3):
        _assert_same(_device_run(case, steps), _host_run(case, steps), steps)


def test_kernels_at_the_largest_batch():
    """n = 1024 at F = 513: 32 whole stages of G in the step, 2 or more frame tiles in the forward"""
    case = ref.make_case((513, 5, 1024, 3))
    _assert_same(_device_run(case, 1), _host_run(case, 1), "n1024")


def test_non_default_stream_and_repeatability():
    case = ref.make_case((513, 40, 65, 6))
    want = _host_run(case, 3)
    side = torch.cuda.Stream()
    first = _device_run(case, 3, stream=side)
    _assert_same(first, want, "side stream")
    _assert_same(_device_run(case, 3, stream=side), first, "twice")
    _assert_same(_device_run(case, 3), first, "default stream")


def test_a_gradient_depends_on_n_alone_and_a_state_on_its_frame_alone():
    case = ref.make_case((12288, 32, 130, 3))
    full = _device_run(case, 1)
    _assert_same(full, _host_run(case, 1), "64x64x3")
    part = _device_run(case, 1, n=3)
    assert ref.same_bits(part[0], full[0][:3])                      # a frame's state does not depend on its batch
    _assert_same(part, _host_run(case, 1, n=3), "n3")


def test_refusals_touch_nothing():
    case = ref.make_case((193, 5, 2, 3))
    F, S = case["V"].shape
    x = torch.from_numpy(case["frames"]).cuda()
    Gd, cd = torch.from_numpy(case["G"]).cuda(), torch.from_numpy(case["c"]).cuda()
    V, m, v, g, states = Guarded((F, S), case["V"]), Guarded((F, S)), Guarded((F, S)), Guarded((F, S)), Guarded((2, S))
    work = Guarded((_lib.linear_srl_workspace_bytes(F, S, 2) // 8,))
    good = ref.adam_at(1)

    def fwd(n=2, F_=F, S_=S, scale=case["scale"], offset=case["offset"], frames=x.data_ptr(), w=None):
        _lib.linear_srl_forward(0, frames, n, F_, S_, scale, offset, V.ptr(), cd.data_ptr(), states.ptr(), work.ptr() if w is None else w)

    def step(n=2, S_=S, adam=good, G=Gd.data_ptr(), scale=case["scale"]):
        _lib.linear_srl_step(0, x.data_ptr(), n, F, S_, scale, case["offset"], G, V.ptr(), m.ptr(), v.ptr(), adam, grad_out_ptr=g.ptr())

    bad_calls = [(lambda: fwd(n=0), -22), (lambda: fwd(n=1025), -95), (lambda: fwd(S_=65), -95), (lambda: fwd(F_=0), -95),
                 (lambda: fwd(scale=np.ones(9), offset=np.ones(9)), -95), (lambda: fwd(scale=np.array([np.inf, 1, 1])), -22),
                 (lambda: fwd(frames=None), -22), (lambda: fwd(w=work.ptr() + 8), -22),
                 (lambda: step(n=-1), -22), (lambda: step(n=2000), -95), (lambda: step(S_=0), -95), (lambda: step(G=None), -22),
                 (lambda: step(adam=dict(good, lr=float("nan"))), -22), (lambda: step(adam=dict(good, beta1=1.0)), -22),
                 (lambda: step(adam=dict(good, eps=-1.0)), -22), (lambda: step(adam=dict(good, bc2=0.0)), -22)]
    for call, code in bad_calls:
        with pytest.raises(_lib.SrlHipError) as e:
            call()
        assert "({})".format(code) in str(e.value) and "linear_srl" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert ref.same_bits(V.get(), case["V"])
    for buf in (m, v, g, states, work):
        assert (buf.get() == SENTINEL).all()


def test_record_train_load_evaluate_rollout(tmp_path):
    """the whole loop on the device.  The assertions are shapes, finiteness and the equality of the hip and host backends' V when both are
    fed the same G — not a learning-quality number."""
    from environments import dataset_generator as dg
    from srlhip.pixel_env import PixelStateVecEnv
    from state_representation import evaluate, linear_srl
    from state_representation.models import SRLLinear, loadSRLModel
    root = str(tmp_path) + "/"
    dg.main(["--num-cpu", "2", "--num-episode", "2", "--save-path", root, "--env", "MobileRobotGymEnv-v0", "--seed", "1", "--name", "mob",
             "--img-size", "64"])
    frames, indices, actions, starts, truth = linear_srl.load_dataset(root + "mob")
    N = len(frames)
    assert frames.shape[1:] == (64, 64, 3) and len(actions) == N and starts.sum() == 2
    trainer = linear_srl.LinearSRLTrainer((64, 64), 3, 4, ["inverse", "forward"], 4, backend="hip", seed=3)
    history = trainer.fit(frames, actions, starts, truth, epochs=1, batch_size=128, seed=3)
    assert trainer.encoder.t == -(-(N - 2) // 128) and np.isfinite(history).all()
    path = trainer.save(root + "logs")
    model = loadSRLModel(path, cuda=True, img_shape=(64, 64))
    assert isinstance(model, SRLLinear) and model.hip is not None and model.backend == "hip"
    V, c = trainer.encoder.weights()
    assert np.isfinite(V).all() and np.isfinite(c).all()
    states = model.getStates(frames[:32]).cpu().numpy()
    want = trainer.encoder.forward(frames[:32]).cpu().numpy()
    assert states.shape == (32, 4) and np.allclose(states, want, rtol=0, atol=1e-9 * max(1.0, np.abs(want).max()))
    out = evaluate.evaluate_model(root + "mob", path, backend="hip", log_folder=root + "logs", frames=frames, indices=indices)
    assert out["n_frames"] == N and np.isfinite(out["knn_mse"]) and out["knn_mse_ground_truth"] <= out["knn_mse"]
    # the hip and host encoders from the same seed, fed the same G for three steps: the same bits in V
    hip = linear_srl.LinearEncoder((64, 64), 3, 4, backend="hip", seed=5)
    host = linear_srl.LinearEncoder((64, 64), 3, 4, backend="host", seed=5)
    rng = np.random.RandomState(0)
    for t in range(3):
        batch = frames[40 * t:40 * t + 33]
        s_hip, s_host = hip.forward(batch).cpu().numpy(), host.forward(batch).numpy()
        assert ref.same_bits(s_hip, s_host)
        G = rng.standard_normal((33, 4)) / 33
        hip.step(batch, G)
        host.step(batch, G)
    assert ref.same_bits(hip.weights()[0], host.weights()[0])
    env = PixelStateVecEnv("MobileRobotGymEnv-v0", 8, model, seed=2, img_shape=(64, 64))
    env.reset()
    weights = torch.from_numpy(rng.standard_normal((8, 4, 4))).cuda()
    roll = env.rollout_policy(5, weights)
    torch.cuda.synchronize()
    assert tuple(roll["obs"].shape) == (5, 8, 4) and bool(torch.isfinite(roll["obs"]).all()) and tuple(roll["reward"].shape) == (5, 8)
    env.close()
