"""A frame's state must not depend on its batch: BIT equality, no tolerance, for both HIP encoders.

Neither kernel reduces across frames or splits a reduction by batch size (every frame is one workgroup's loop iteration in
csrc/encoder.hip, a set of workgroups of its own in csrc/encoder_general.hip; no floating-point atomics), so every situation below must
give the bits of the same frame in a batch of the 8 pool frames (tests/encoder_ref.py: frame_pool).  The situations
(tests/encoder_gpu_common.py: situations): each pool frame alone, first / in the middle / last in batches of the sizes below, among other
neighbours, after the handle served a larger and then a smaller batch, on a side stream, and replayed twice from a HIP graph
(srlhip_graph_begin / _end / _launch around one srlhip_encoder_forward on an env handle's stream) with the frame buffer refilled between
the replays.

Batch sizes.  Fused 64x64x3: the grid is min(n, CUs) workgroups (fused_launch), CUs = torch's multi_processor_count = the
multiProcessorCount the library reads: n = 1, 2, CUs - 1, CUs, CUs + 1 (the first workgroup takes a second, prefetched frame, the others
end after one), 2 CUs + 3 (a third turn for three workgroups).  Layered path: one launch covers up to 32768 frames (general_forward:
kChunk, grid.z) and the batch's last frame reads its last pixel differently (enc_layer_k: `tail`); inside a launch the number of bands a
layer-2 / layer-3 workgroup walks — with the next band's window prefetched behind the current one — is
clamp(nbands * nsegs * n / 4096, 1, nbands) (bands_per_wg): the sizes are 2, 3, 9, both sides of every n at which that count changes, and
for 48x56x3 32768 and 32769 (positions: first, the last frame of the first launch, last).  224x224x3: n = 1 and 3 only."""
import pytest
import torch

import encoder_gpu_common as common
import encoder_ref as ref

pytestmark = pytest.mark.gpu


def report(bad):
    return "%d records differ from the frame's bits in the batch of 8, e.g. %s" % (len(bad), bad[:6])


def band_sizes(shape, ch):
    """both sides of every batch size at which bands_per_wg of layer 2 or 3 changes (csrc/encoder_pack.hpp: geometry; kR2 = 2, kR3 = 1
    pooled rows per band, 15 pooled columns per segment)"""
    h, w = shape
    hc, wc = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
    hp, wp = [(hc + 2 - 3) // 2 + 1], [(wc + 2 - 3) // 2 + 1]
    for stride in (1, 2):
        hc, wc = (hp[-1] + 2 - 3) // stride + 1, (wp[-1] + 2 - 3) // stride + 1
        hp.append((hc - 3) // 2 + 1); wp.append((wc - 3) // 2 + 1)
    sizes = set()
    for layer, rows in ((1, 2), (2, 1)):
        nbands, nsegs = (hp[layer] + rows - 1) // rows, (wp[layer] + 14) // 15
        for k in range(2, nbands + 1):
            n = -(-4096 * k // (nbands * nsegs))
            sizes |= {n - 1, n}
    return sizes


def test_band_sizes_are_where_the_count_changes():
    assert band_sizes((48, 56), 3) == {2730, 2731, 4095, 4096}
    assert band_sizes((64, 64), 6) == {2047, 2048, 3071, 3072, 4095, 4096}
    assert {1638, 1639, 4095, 4096} <= band_sizes((75, 61), 3)


def test_fused_default_path():
    cus, sizes = common.fused_sizes()
    net = common.hip_net(ref.fresh_state_dict(3, 23), (64, 64), 3)
    rec = common.situations(net, (64, 64), 3, sizes, cus + 1, cus + 1)
    bad = common.mismatches(rec)
    assert not bad, report(bad)
    assert not net.hip.overflow()


@pytest.mark.parametrize("knob,value", [("SRLHIP_ENCODER_L1", "f16"), ("SRLHIP_ENCODER_WAVES", "8")])
def test_fused_variant_in_a_child_process(knob, value):
    rec = common.run_child(knob, value)[0]
    assert len(rec) > 8 * 20
    bad = common.mismatches(rec)
    assert not bad, report(bad)


def test_the_variants_are_other_arithmetic_than_the_default():
    """the two knobs reached the library: the split-f16 layer 1 rounds differently from the int8 layer 1, so the children's base bits
    differ from the default path's somewhere (and the two f16 forms, one and two waves per SIMD, sum in another order)"""
    net = common.hip_net(ref.fresh_state_dict(3, 23), (64, 64), 3)
    pool = ref.frame_pool((64, 64), 3)
    default = [row.tobytes().hex() for row in net.getStates(pool).cpu().numpy()]
    f16 = [bits for name, i, bits in common.run_child("SRLHIP_ENCODER_L1", "f16")[0] if name == "base"]
    assert f16 != default


@pytest.mark.parametrize("shape,ch,l1", [((48, 56), 3, None), ((48, 56), 3, "i8"), ((75, 61), 3, None), ((64, 64), 6, None)])
def test_layered_path(shape, ch, l1, monkeypatch):
    if l1:
        monkeypatch.setenv("SRLHIP_ENCODER_L1", l1)         # read when the handle is created
    net = common.hip_net(ref.fresh_state_dict(3, 29, shape, ch), shape, ch)
    sizes = {2, 3, 9} | band_sizes(shape, ch)
    if shape == (48, 56) and not l1:
        sizes |= {common.CHUNK, common.CHUNK + 1}
    rec = common.situations(net, shape, ch, sizes, 9, 9)
    bad = common.mismatches(rec)
    assert not bad, report(bad)
    assert not net.hip.overflow()


def test_layered_path_at_224():
    """n = 1 and 3 only, each pool frame alone, first and last; no graph, no large batches"""
    shape, ch = (224, 224), 3
    net = common.hip_net(ref.fresh_state_dict(3, 31, shape, ch), shape, ch)
    pool = torch.from_numpy(ref.frame_pool(shape, ch)).cuda()
    base = net.getStates(pool).cpu().numpy()
    assert len({row.tobytes() for row in base}) == 8
    bad = []
    filler = torch.randint(0, 256, (3,) + shape + (ch,), dtype=torch.uint8, device="cuda")
    for r in range(8):
        alone = net.getStates(pool[r:r + 1]).cpu().numpy()
        batch = filler.clone()
        batch[0], batch[2] = pool[r], pool[(r + 1) % 8]
        three = net.getStates(batch).cpu().numpy()
        for name, i, row in (("alone", r, alone[0]), ("first of 3", r, three[0]), ("last of 3", (r + 1) % 8, three[2])):
            if row.tobytes() != base[i].tobytes():
                bad.append((name, i, row.tobytes().hex(), base[i].tobytes().hex()))
    assert not bad, report(bad)
