"""Generate tests/golden/cnn_policy_reference.npz by running the REFERENCE's own CNNPolicyPytorch
(/root/reference/rl_baselines/evolution_strategies/cma_es.py) through PytorchPolicy.setParam / getActionProba on the CPU, with the
modules its file imports but this never calls (`cma`, rl_baselines.base_classes, rl_baselines.utils) stubbed.

Run in the build container only:   python tests/golden/make_cnn_policy_golden.py
The .npz is committed (data only); tests never need /root/reference.

Recorded: the parameter vectors, two structured 224x224x3 frames and two 64x64x6 frames (A = 6), the float32 outputs of the module as
CMA-ES drives it (continuous_actions=True: the scores themselves; and the softmax probabilities of the discrete form), and the outputs of
the same module in .double() on obs / 255.0 in float64.  At 64x64 the reference's fc layer (288 inputs) does not fit: the script's own
subclass replaces that one layer by the Linear(F, A) the frame size needs, everything else is the reference's text.
This pins the parameter order (vector_to_parameters), the training-mode batch-norm on a batch of one and the NHWC -> NCHW step."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cnn_policy_ref as ref  # noqa: E402


def load_reference():
    for name, attrs in (("cma", {}), ("rl_baselines", {}), ("rl_baselines.base_classes", {"BaseRLObject": object}),
                        ("rl_baselines.utils", {"createEnvs": None})):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("reference_cma_es", "/root/reference/rl_baselines/evolution_strategies/cma_es.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    cma_es = load_reference()

    class SmallFrameCNN(cma_es.CNNPolicyPytorch):
        def __init__(self, in_dim, out_dim, features):
            super(SmallFrameCNN, self).__init__(in_dim, out_dim)
            self.fc = torch.nn.Linear(features, out_dim)

    rng = np.random.RandomState(20260)
    out, A = {}, 6
    for tag, (H, W, C) in (("224", (224, 224, 3)), ("64", (64, 64, 6))):
        F = ref.shape(C, H, W)[2]
        frames = ref.structured_frames(rng, 2, H, W, C)
        params = ref.random_params(rng, C, H, W, A, 2, flavour="signs")
        net = cma_es.CNNPolicyPytorch(C, A) if F == 288 else SmallFrameCNN(C, A, F)
        scores, proba, scores64 = [], [], []
        for e in range(2):
            pol = cma_es.PytorchPolicy(net, True, srl_model=False, cuda=False, deterministic=True)
            assert pol.getParamSpace() == params.shape[1], (pol.getParamSpace(), params.shape)
            pol.setParam(params[e])
            # this torch keeps the transposed observation's strides through the convolutions, where the module's .view() then fails:
            # hand the module the same values in a contiguous tensor
            pol.toTensor = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(torch.float)
            scores.append(pol.getActionProba(np.array([frames[e]]))[0])
            pol.continuous_actions = False
            proba.append(pol.getActionProba(np.array([frames[e]]))[0])
            net.double()
            with torch.no_grad():
                x = torch.from_numpy(np.ascontiguousarray(np.transpose(np.array([frames[e]]) / 255.0, (0, 3, 1, 2))))
                scores64.append(net(x)[0].numpy().copy())
            net.float()
        out["frames_" + tag], out["params_" + tag] = frames, params
        out["scores_" + tag] = np.array(scores, dtype=np.float32)
        out["proba_" + tag] = np.array(proba, dtype=np.float32)
        out["scores64_" + tag] = np.array(scores64, dtype=np.float64)
    path = os.path.join(HERE, "cnn_policy_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
