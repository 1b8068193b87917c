"""tests/encoder_ref.py without a GPU: the float64 forward is pinned to the existing float32 CPU forward on every input the GPU encoder tests
use, and the overflow cases are shown to sit on the intended sides of 65504 by the float64 forward alone.  Prints the E32 table
(E32 = max|f32 - f64| / max|f64| per case) and the (a) / (b) predictions; the GPU tests recompute E32 from the same inputs."""
import numpy as np
import pytest

import encoder_ref as ref


def check(name, sd, imgs):
    s64, maxima = ref.forward64(sd, imgs)
    s32 = ref.forward32(sd, imgs)
    assert s64.dtype == np.float64 and s32.dtype == np.float32 and s64.shape == s32.shape
    assert np.isfinite(s32).all() and np.isfinite(s64).all() and np.isfinite(maxima).all(), name
    e32 = ref.rel_err(s32, s64)
    print("E32 %-28s n %3d  max|f64| %10.4g  E32 %.3e  pooled maxima %s" % (name, len(imgs), np.abs(s64).max(), e32, np.array2string(maxima, precision=4)))
    # a family that breaks the float32 reference is not a test of the kernel
    assert e32 < ref.E32_SANE, (name, e32)
    # no watched layer is anywhere near float16's range on its own: the flag must stay clear in the accuracy tests
    assert max(maxima[l - 1] for l in ref.WATCHED) < ref.F16_MAX / 4, (name, maxima)
    return e32


@pytest.mark.parametrize("name", ref.FAMILY_CASE_NAMES)
def test_float64_forward_pins_the_float32_forward_on_the_weight_families(name):
    check(name, *ref.family_case(name))


@pytest.mark.parametrize("state_dim,n", ref.EXISTING_FUSED)
def test_float64_forward_on_the_existing_fused_cases(state_dim, n):
    check("fused sd%d n%d" % (state_dim, n), *ref.existing_fused_case(state_dim, n))


@pytest.mark.parametrize("shape,ch,state_dim,n", ref.EXISTING_LAYERED)
def test_float64_forward_on_the_existing_layered_cases(shape, ch, state_dim, n):
    check("layered %dx%dx%d sd%d" % (shape[0], shape[1], ch, state_dim), *ref.existing_layered_case(shape, ch, state_dim, n))


def test_float64_forward_is_the_unfolded_module_and_sees_every_frame_alone():
    """forward64 is batch-independent itself (frame i of a batch = frame i alone, to float64 rounding of a different blocking) and its
    maxima are the maxima over the frames"""
    sd, imgs = ref.family_case("negbn 48x56x3 sd3")
    s, m = ref.forward64(sd, imgs)
    alone = [ref.forward64(sd, imgs[i:i + 1]) for i in range(len(imgs))]
    assert np.abs(np.concatenate([a[0] for a in alone]) - s).max() <= 1e-12 * np.abs(s).max()
    assert np.allclose(np.max([a[1] for a in alone], axis=0), m, rtol=1e-12)
    # negated BatchNorm weights really flip channels: the pooled maximum is not the pooled maximum of the un-negated network
    assert not np.allclose(m, ref.forward64(ref.family_state_dict("fresh", 3, (48, 56), 3), imgs)[1])


@pytest.mark.parametrize("shape,ch", ref.OVERFLOW_SHAPES)
@pytest.mark.parametrize("layer", (1, 2, 3))
def test_overflow_cases_sit_on_the_intended_sides(shape, ch, layer):
    """(a): the layer's pooled pre-activation maximum is 65504 / 2, (b): 2 * 65504, to float32 rounding of the scaled BatchNorm; every
    other layer's maximum and the states are what they were (the next layer undoes the factor), so a flag can only come from `layer`"""
    sd, imgs = ref.overflow_base(shape, ch)
    s0, m0 = ref.forward64(sd, imgs)
    sides = {}
    for side, target in (("a", ref.F16_MAX / 2), ("b", ref.F16_MAX * 2)):
        sd2 = ref.overflow_state_dict(sd, imgs, layer, side)
        s, m = ref.forward64(sd2, imgs)
        e32 = ref.rel_err(ref.forward32(sd2, imgs), s)
        print("OVERFLOW %dx%dx%d layer %d (%s): pooled maximum %.3f (target %.1f), others %s, E32 %.3e" %
              (shape[0], shape[1], ch, layer, side, m[layer - 1], target, np.array2string(np.delete(m, layer - 1), precision=4), e32))
        assert abs(m[layer - 1] / target - 1.0) < 1e-5
        others = [l for l in (1, 2, 3) if l != layer]
        assert np.allclose(m[[l - 1 for l in others]], m0[[l - 1 for l in others]], rtol=1e-5)
        assert max(m[l - 1] for l in ref.WATCHED if l != layer) < ref.F16_MAX / 4
        assert ref.rel_err(s, s0) < 1e-5                  # the same function of the frame, but for float32 rounding of the moved weights
        assert e32 < ref.E32_SANE
        sides[side] = m[layer - 1]
    assert sides["a"] < 0.51 * ref.F16_MAX and sides["b"] > 1.9 * ref.F16_MAX
    assert sides["b"] == 4.0 * sides["a"]                 # the two sides differ by a power of two: exact in float64
