"""Both HIP encoders against the float64 forward of tests/encoder_ref.py, with the bar set by the reference's own error:
E_kernel = max|kernel - f64| / max|f64| <= 4 x E32, E32 = max|f32 CPU forward - f64| / max|f64| of the same case (no floor of 1 under the
denominator; encoder_ref.py: THE BAR).  Cases: the five weight families at the fused shape and three layered shapes (and two at
224x224x3), the five fused and seven layered parametrisations of tests/test_gpu_encoder.py / test_gpu_encoder_general.py, the layered
int8 layer 1, and the fused kernel's two experiment variants (child processes).  Every case prints both figures; the table measured on an
MI355X is in profiles/NOTES.md (section "Encoder error against float64").

Losing the lo half of one operand costs about 2^-11 = 4.9e-4: three orders of magnitude over the bar."""
import pytest

import encoder_gpu_common as common
import encoder_ref as ref

pytestmark = pytest.mark.gpu


def hold(name, sd, imgs):
    (_, ek, e32, flag), = common.errors([(name, sd, imgs)])
    print("ERR %-30s E_kernel %.3e  E32 %.3e  ratio %.2f" % (name, ek, e32, ek / e32))
    assert e32 < ref.E32_SANE
    assert not flag
    assert ek <= ref.BAR * e32, (name, ek, e32)


@pytest.mark.parametrize("name", ref.FAMILY_CASE_NAMES)
def test_weight_families(name):
    hold(name, *ref.family_case(name))


@pytest.mark.parametrize("state_dim,n", ref.EXISTING_FUSED)
def test_existing_fused_cases(state_dim, n):
    hold("fused sd%d n%d" % (state_dim, n), *ref.existing_fused_case(state_dim, n))


@pytest.mark.parametrize("shape,ch,state_dim,n", ref.EXISTING_LAYERED)
def test_existing_layered_cases(shape, ch, state_dim, n):
    hold("layered %dx%dx%d sd%d" % (shape[0], shape[1], ch, state_dim), *ref.existing_layered_case(shape, ch, state_dim, n))


@pytest.mark.parametrize("name", [n for n in ref.FAMILY_CASE_NAMES if " 48x56x3 " in n or " 75x61x3 " in n])
def test_weight_families_on_the_layered_int8_layer_1(name, monkeypatch):
    monkeypatch.setenv("SRLHIP_ENCODER_L1", "i8")           # read when the handle is created
    hold("i8 " + name, *ref.family_case(name))


@pytest.mark.parametrize("knob,value", [("SRLHIP_ENCODER_L1", "f16"), ("SRLHIP_ENCODER_WAVES", "8")])
def test_weight_families_on_the_fused_variants(knob, value):
    errs = common.run_child(knob, value)[3]
    assert [e[0] for e in errs] == [c[0] for c in common.fused_family_cases()]
    for name, ek, e32, flag in errs:
        print("ERR %s=%s %-24s E_kernel %.3e  E32 %.3e  ratio %.2f" % (knob, value, name, ek, e32, ek / e32))
    for name, ek, e32, flag in errs:
        assert not flag and ek <= ref.BAR * e32, (name, ek, e32)
