"""The SRL encoder's forward in float64 — the DEFINITION the two HIP encoders (csrc/encoder.hip, csrc/encoder_general.hip) are measured
against — with the inputs the encoder tests share: the frame pool, the weight families and the overflow cases.

forward64() is the torch module itself (state_representation/models.py: CustomCNN) run under .double() on the CPU from the same
state_dict: preprocess as SRLNeuralNetwork.getStates does (/255, ImageNet mean / std, H and W swapped), then conv / BatchNorm (eval) / ReLU /
max-pool / FC.  No BatchNorm folding, no operand splitting, no restatement of how the kernels tile the work.  Next to the states it returns,
per layer, the largest POOLED PRE-ACTIVATION: max over frames, channels and pooled pixels of maxpool(BN(conv(x))) — the value the
kernels' overflow watch sees before its ReLU (the watch looks at max(0, that)).

THE BAR.  E32 = max|f32 - f64| / max|f64| over all frames and state components of a case, f32 the existing float32 CPU forward
(SRLNeuralNetwork(cuda=False, backend="torch").getStates: PyTorch's float32 convolutions on BatchNorm-folded weights — the same folded
float32 weights the kernels are given).  A kernel is held to E_kernel = max|kernel - f64| / max|f64| <= BAR * E32 of the same case, no floor
of 1 under the denominator.  BAR = 4 is the factor tests/cnn_policy_ref.py (SCORE_TOL) gives a kernel that sums the same terms in another
order.  E32 is measured where the test runs, from the same inputs, never pinned from what a kernel gave.

THE OVERFLOW CASES.  overflow_state_dict() moves ONE layer's pooled pre-activation maximum to 65504 / 2 or 2 * 65504 and leaves every
other layer's input as it was: the layer's BatchNorm weight and bias are multiplied by c (its output scales by c exactly in real
arithmetic) and the next layer's convolution (or the FC) weights by 1 / c.  c = float32(65504 / max) * 2^(-1 | +1): the first factor defines
a base network once (its float32 rounding is part of that network's definition), the power of two is exact in float32 and float64, so the
float64 maxima of the two sides are exactly a quarter apart and sit within float32 rounding of 32752 and 131008."""
import numpy as np
import torch

from state_representation.models import IMAGENET_MEAN, IMAGENET_STD, CustomCNN, SRLNeuralNetwork

F16_MAX = 65504.0
BAR = 4.0                       # E_kernel <= BAR * E32 (tests/cnn_policy_ref.py: SCORE_TOL = 4 * E32)
E32_SANE = 1e-4                 # a family whose float32 CPU forward is further than this from float64 tests the reference, not the kernel
CONV, BN, POOL = (0, 4, 8), (1, 5, 9), (3, 7, 11)        # indices into CustomCNN.conv_layers
WATCHED = (1, 2)                # layers whose pooled activations travel as f16 hi / lo planes (both kernels keep layer 3's features in float32)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def preprocess64(images_u8):
    x = torch.from_numpy(np.ascontiguousarray(images_u8)).to(torch.float64) / 255.0
    c = x.shape[-1]
    mean = torch.tensor(IMAGENET_MEAN * (c // 3), dtype=torch.float64)
    std = torch.tensor(IMAGENET_STD * (c // 3), dtype=torch.float64)
    return ((x - mean) / std).permute(0, 3, 2, 1).contiguous()


def forward64(state_dict, images_u8):
    """-> (states float64 [n][state_dim], maxima float64 [3]: the largest pooled pre-activation of layers 1..3)"""
    n, H, W, C = images_u8.shape
    state_dim = state_dict["fc.weight"].shape[0]
    model = CustomCNN(state_dim, C, (H, W))
    model.load_state_dict(state_dict)
    model = model.double().eval()
    maxima = []
    with torch.no_grad():
        x = preprocess64(images_u8)
        for l in range(3):
            y = model.conv_layers[BN[l]](model.conv_layers[CONV[l]](x))
            pool = model.conv_layers[POOL[l]]
            maxima.append(float(pool(y).max()))
            x = pool(torch.relu(y))
        out = model.fc(x.reshape(n, -1))
    return out.numpy(), np.array(maxima)


def forward32(state_dict, images_u8):
    """the existing float32 CPU forward of the same network -> float32 [n][state_dim]"""
    n, H, W, C = images_u8.shape
    cpu = SRLNeuralNetwork(state_dict["fc.weight"].shape[0], cuda=False, img_shape=(H, W), n_channels=C, state_dict=state_dict, backend="torch")
    return cpu.getStates(images_u8).numpy()


def rel_err(out, ref64):
    """max|out - f64| / max|f64|: no floor under the denominator"""
    ref64 = np.asarray(ref64, dtype=np.float64)
    return float(np.abs(np.asarray(out, dtype=np.float64) - ref64).max() / np.abs(ref64).max())


# ---- frames -----------------------------------------------------------------------------------------------------------------------------
def frame_pool(shape, ch):
    """8 distinct uint8 frames [8][H][W][ch]: three random, all 0, all 255, random with a flat block, a render-like one (flat floor,
    gradient, rectangles: stands in for a rasterised frame without a GPU), random with a flat zero border"""
    H, W = shape
    rs = np.random.RandomState(1000 + 7 * H + W + ch)
    p = rs.randint(0, 256, size=(8, H, W, ch)).astype(np.uint8)
    p[3] = 0
    p[4] = 255
    p[5, H // 6:H // 2, W // 8:3 * W // 4] = rs.randint(0, 256, size=ch).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for c in range(ch):
        img = 60.0 + (40.0 * c) % 97 + 80.0 * yy / H + 30.0 * np.sin(xx / (3.0 + c))
        for _ in range(4):
            y0, x0 = rs.randint(H - 4), rs.randint(W - 4)
            img[y0:y0 + rs.randint(3, max(4, H // 3)), x0:x0 + rs.randint(3, max(4, W // 3))] = rs.randint(256)
        p[6, :, :, c] = np.clip(img, 0, 255).astype(np.uint8)
    p[7, :, :W // 3] = 0
    assert len({f.tobytes() for f in p}) == 8
    return p


def case_frames(shape, ch, n):
    """the pool, then random frames up to n"""
    pool = frame_pool(shape, ch)
    if n <= 8:
        return pool[:n].copy()
    rs = np.random.RandomState(n + shape[0])
    return np.concatenate([pool, rs.randint(0, 256, size=(n - 8,) + tuple(shape) + (ch,)).astype(np.uint8)])


# ---- weights ----------------------------------------------------------------------------------------------------------------------------
def fresh_state_dict(state_dim, seed, img_shape=(64, 64), n_channels=3):
    """default initialisation with perturbed BatchNorm statistics — the same draws, in the same order, as make_net / make_nets of
    tests/test_gpu_encoder.py and tests/test_gpu_encoder_general.py"""
    torch.manual_seed(seed)
    net = SRLNeuralNetwork(state_dim, img_shape=img_shape, n_channels=n_channels, backend="torch")
    for m in net.model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.5); m.running_var.uniform_(0.5, 2.0); m.weight.data.uniform_(0.5, 1.5); m.bias.data.normal_(0, 0.2)
    return {k: v.detach().clone() for k, v in net.model.state_dict().items()}


FAMILIES = ("fresh", "spread", "negbn", "dead_dom", "fcrows")


def family_state_dict(family, state_dim, img_shape, n_channels, seed=5):
    """fresh:    default initialisation, perturbed BatchNorm statistics
    spread:   every conv layer's output channels multiplied by 2^u, u uniform in [-8, 4] (the packer's one power-of-two scale per layer
              meets channels 4096 x apart)
    negbn:    BatchNorm weight negated on a third of each layer's channels (folding flips the sign of the whole channel: pooling the raw
              accumulators before the affine must pool the right extreme)
    dead_dom: per layer one channel with all-zero weights — in layer 1 with zero folded bias too, an all-zero row for the packers — and
              one channel whose BatchNorm bias (40) dominates its convolution
    fcrows:   FC rows multiplied by 2^u, u uniform in [-8, 8]"""
    assert family in FAMILIES
    sd = fresh_state_dict(state_dim, seed, img_shape, n_channels)
    rs = np.random.RandomState(100 + FAMILIES.index(family))
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    if family == "spread":
        for l in range(3):
            sd["conv_layers.%d.weight" % CONV[l]] *= f32(2.0 ** rs.uniform(-8, 4, size=64)).view(-1, 1, 1, 1)
    elif family == "negbn":
        for l in range(3):
            sd["conv_layers.%d.weight" % BN[l]][torch.from_numpy(rs.permutation(64)[:21])] *= -1.0
    elif family == "dead_dom":
        for l in range(3):
            d, k = rs.choice(64, size=2, replace=False)
            sd["conv_layers.%d.weight" % CONV[l]][d] = 0.0
            if l == 0:
                sd["conv_layers.%d.running_mean" % BN[l]][d] = 0.0
                sd["conv_layers.%d.bias" % BN[l]][d] = 0.0
            sd["conv_layers.%d.bias" % BN[l]][k] = 40.0
    elif family == "fcrows":
        sd["fc.weight"] *= f32(2.0 ** rs.uniform(-8, 8, size=state_dim)).view(-1, 1)
    return sd


SHAPES = (((64, 64), 3), ((48, 56), 3), ((75, 61), 3), ((64, 64), 6))     # the fused shape and the layered shapes of the invariance test


# every family at every shape of SHAPES with 12 frames (the pool + 4 random), state_dim 3 and 64 alternating; fresh and spread also at
# 224 x 224 x 3 with 3 frames
FAMILY_CASE_NAMES = tuple("%s %dx%dx%d sd%d" % (fam, s[0], s[1], c, (3, 64)[(fi + si) % 2])
                          for fi, fam in enumerate(FAMILIES) for si, (s, c) in enumerate(SHAPES)) + ("fresh 224x224x3 sd3", "spread 224x224x3 sd3")


def family_case(name):
    fam, shp, sdim = name.split()
    H, W, C = (int(v) for v in shp.split("x"))
    n = 3 if H == 224 else 12
    return family_state_dict(fam, int(sdim[2:]), (H, W), C), case_frames((H, W), C, n)


# the parametrisations of the two existing GPU test files, restated: (state_dim, n) of test_hip_encoder_matches_torch_fp32 and
# (shape, channels, state_dim, n) of test_layered_encoder_matches_torch_fp32
EXISTING_FUSED = ((3, 1), (5, 37), (2, 600), (200, 64), (300, 5))
EXISTING_LAYERED = (((224, 224), 3, 3, 5), ((64, 64), 6, 5, 37), ((224, 224), 6, 2, 3), ((96, 128), 3, 4, 9), ((128, 96), 6, 200, 4), ((75, 61), 3, 3, 6),
                    ((48, 56), 3, 2, 70))


def existing_fused_case(state_dim, n):
    rs = np.random.RandomState(n)
    imgs = rs.randint(0, 256, size=(n, 64, 64, 3)).astype(np.uint8)
    imgs[0, :, :20] = 0
    if n > 2:
        imgs[1] = 255
        imgs[2, 10:50, 5:60] = rs.randint(0, 256, size=3).astype(np.uint8)
    return fresh_state_dict(state_dim, 7 + state_dim), imgs


def existing_layered_case(shape, ch, state_dim, n):
    rs = np.random.RandomState(n)
    imgs = rs.randint(0, 256, size=(n,) + tuple(shape) + (ch,)).astype(np.uint8)
    imgs[0, :, :shape[1] // 3] = 0
    if n > 2:
        imgs[1] = 255
        imgs[2, shape[0] // 6:, : shape[1] // 2] = rs.randint(0, 256, size=ch).astype(np.uint8)
    return fresh_state_dict(state_dim, 11 + state_dim, shape, ch), imgs


# ---- the overflow flag ------------------------------------------------------------------------------------------------------------------
OVERFLOW_SHAPES = (((64, 64), 3), ((48, 56), 3))          # the fused path and one layered shape


def overflow_state_dict(state_dict, images_u8, layer, side):
    """`layer` 1..3; side "a": that layer's pooled pre-activation maximum over images_u8 becomes 65504 / 2, "b": 2 * 65504 (see the
    module docstring).  -> a new state_dict"""
    assert layer in (1, 2, 3) and side in ("a", "b")
    m = forward64(state_dict, images_u8)[1][layer - 1]
    assert m > 0.0, "the layer's pooled maximum must be positive to be moved by a positive factor"
    c = np.float32(F16_MAX / m) * np.float32(0.5 if side == "a" else 2.0)
    assert np.isfinite(c) and c > 0
    sd = {k: v.detach().clone() for k, v in state_dict.items()}
    sd["conv_layers.%d.weight" % BN[layer - 1]] *= float(c)
    sd["conv_layers.%d.bias" % BN[layer - 1]] *= float(c)
    nxt = "conv_layers.%d.weight" % CONV[layer] if layer < 3 else "fc.weight"
    sd[nxt] *= float(np.float32(1.0) / c)
    return sd


def overflow_base(shape, ch):
    """the network and the frames the overflow cases start from: fresh weights, state_dim 3, the pool"""
    return fresh_state_dict(3, 17, shape, ch), frame_pool(shape, ch)
