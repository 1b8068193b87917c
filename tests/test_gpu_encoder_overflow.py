"""srlhip_encoder_overflow on both sides of the line, for every layer the kernels watch.

Both kernels carry the pooled activations of layers 1 and 2 between layers as float16 hi / lo planes and watch them (csrc/encoder.hip:
the int8 layer 1's `mx`, store_split's `ovf`; csrc/encoder_general.hip: emit); layer 3's pooled features stay float32 and are NOT watched.
tests/encoder_ref.py (overflow_state_dict) moves one layer's pooled pre-activation maximum to (a) 65504 / 2 or (b) 2 x 65504 with every
other layer's input unchanged; tests/test_encoder_ref_cpu.py shows with the float64 forward alone that the cases sit there.
  (a) layers 1, 2: the flag stays clear and the states hold the bar of tests/test_gpu_encoder_f64.py (E_kernel <= 4 x E32);
  (b) layers 1, 2: the flag is set after the forward;
  layer 3, (a) and (b): the flag stays clear and the bar holds — the features are float32.
The flag is sticky (include/srlhip.h): it stays set across a clean forward through the same handle and reading it does not clear it; a
new handle starts clear.  Runs on the fused path (default int8 layer 1; the split-f16 layer 1 and the two-waves form in their child
processes — their layer-1 watch is other code) and on the layered 48x56x3 shape (split-f16 and int8 layer 1)."""
import pytest

import encoder_gpu_common as common
import encoder_ref as ref

pytestmark = pytest.mark.gpu


def judge(label, flags, persist):
    for (layer, side), (flag, ek, e32, clear_before) in sorted(flags.items()):
        print("FLAG %s layer %d (%s): flag %d  E_kernel %.3e  E32 %.3e" % (label, layer, side, flag, ek, e32))
    for (layer, side), (flag, ek, e32, clear_before) in sorted(flags.items()):
        assert clear_before, "a new handle starts with the flag clear"
        if layer in ref.WATCHED and side == "b":
            assert flag, (label, layer, side)
        else:
            assert not flag, (label, layer, side)
            assert ek <= ref.BAR * e32, (label, layer, side, ek, e32)
    assert persist == (True, True, True), "set by the overflowing forward, kept across a clean forward, kept by the read"


@pytest.mark.parametrize("shape,ch,l1", [((64, 64), 3, None), ((48, 56), 3, None), ((48, 56), 3, "i8")])
def test_flag_on_both_sides_of_the_line(shape, ch, l1, monkeypatch):
    assert (shape, ch) in ref.OVERFLOW_SHAPES
    if l1:
        monkeypatch.setenv("SRLHIP_ENCODER_L1", l1)         # layered path: read when the handle is created
    flags, persist = common.flag_runs(shape, ch)
    judge("%dx%dx%d%s" % (shape[0], shape[1], ch, " i8" if l1 else ""), flags, persist)


@pytest.mark.parametrize("knob,value", [("SRLHIP_ENCODER_L1", "f16"), ("SRLHIP_ENCODER_WAVES", "8")])
def test_flag_on_the_fused_variants(knob, value):
    _, flags, persist, _ = common.run_child(knob, value)
    assert len(flags) == 6
    judge("%s=%s" % (knob, value), flags, persist)
