"""-m gpu: the random generators of the kernels ON THE DEVICE (srlhip_selftest_rng: csrc/rng_probe.hip over csrc/rng.hpp and
csrc/kuka_group.hpp), word for word against numpy's RandomState and the Philox4x32-10 definition — the programs and replays of
tests/test_rng_streams_cpu.py (tests/rng_stream_ref.py).

Exact, no tolerance: seeding, raw words, double01, uniform, bounded, the words / counters each program consumes, the persisted
state, the agreement of an env's 16 lanes, and loc + scale z as the unfused double result of the device's own deviate z.

The VALUE of a Gaussian deviate goes through the device math library's log / sqrt (/ cos), not libm's.  Every deviate drawn in
this file is held to the 200-bit value of sqrt(-2 log(r2) / r2) x (Philox: sqrt(-2 log(u1)) cos(fl(2 pi u2))) computed from the
exact doubles in front of the transcendental functions, within: the worst error of the reference on the same draws (numpy's
own deviates for MT19937, oracle/philox.h through libm for Philox) plus 1 ulp — the device's log and cos are specified to about
1 ulp where libm's are about 0.5; the division, square root and product round the same way on both sides.  How many deviates
differ from the reference's bits, and the worst errors, are printed (DESIGN.md records them).

Measured on an MI355X over every deviate of this file: MT19937 forms 52 of 4068 deviates (1.28 %) differ from numpy's bits, worst
error 1.93 ulp (numpy's own worst on the same draws: 1.62 ulp); Philox forms 115 of 2928 (3.93 %) differ from oracle/philox.h
through libm, worst 1.67 ulp (the oracle's own: 1.67 ulp).  The share is not zero, so equality of the Gaussian values is NOT
asserted here; it is on the host (tests/test_rng_streams_cpu.py)."""
import numpy as np
import pytest

import rng_stream_ref as R
import test_rng_streams_cpu as C

pytestmark = pytest.mark.gpu

TALLY = {"MT19937": R.GaussTally(), "Philox": R.GaussTally()}


@pytest.fixture(scope="module")
def probe():
    return R.device_probe()


def hold_gaussians(t, exact_fn, replays, z_out, v_out):
    """adds the Gaussian draws of these envs to the test's tally `t` (and holds loc + scale z exactly)"""
    for e, rp in enumerate(replays):
        if rp is not None:
            R.check_gaussians(rp, exact_fn, z_out[e, 0], v_out[e, 0], t)


def finish(t, family, what):
    """the bound, over the draws of one test: the reference's worst error on these draws + 1 ulp"""
    print(t.line(what))
    TALLY[family].merge(t)
    assert t.n > 0 and t.got_worst <= t.ref_worst + 1.0, t.line(what)


def exact_but_gaussians(gen, program, out, replays):
    """every value that is not a Gaussian draw: equal; -> nothing"""
    keep = np.array([op != R.NORMAL for op, _ in R.value_ops(gen, program)])
    for e, rp in enumerate(replays):
        got, want = out[e, 0][keep], np.array(rp.values, dtype=np.uint64)[keep]
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (R.GEN_NAMES[gen], "env", e, "first differing value (of the non-Gaussian ones)", int(bad[0]))


def check_mt_device(probe, gen, program, keys, lens, skip, stride, what, min_words=0, min_twists=0):
    v, state = R.run(probe, gen, program, keys, lens, skip=skip, stride=stride)
    z, state_z = R.run(probe, gen, program, keys, lens, skip=skip, stride=stride, std_normals=True)
    C.assert_lanes_agree(v)
    C.assert_lanes_agree(z)
    replays = []
    for e in range(len(keys)):
        rp = R.MtReplay(R.key_list(keys, lens, e))
        rp.skip(int(skip[e]))
        rp.run(program)
        assert rp.words >= min_words and rp.twists >= min_twists, (e, rp.words, rp.twists)
        replays.append(rp)
    exact_but_gaussians(gen, program, v, replays)
    exact_but_gaussians(gen, program, z, replays)
    t = R.GaussTally()
    hold_gaussians(t, R.mt_deviate_exact, replays, z, v)
    for e, rp in enumerate(replays):                           # words, index, has_gauss: exact; the cached deviate: the device's own
        want = rp.state_row()
        assert np.array_equal(state[e][:R.MT_N + 2], want[:R.MT_N + 2]), (R.GEN_NAMES[gen], "state of env", e)
        assert np.array_equal(state_z[e], state[e])
        if want[R.MT_N + 1]:
            x, r2 = rp._pending                              # drawn, not handed out yet: held like the others
            t.add(R.mt_deviate_exact(x, r2), float(R.as_f64(want[R.MT_N + 2:])[0]), float(R.as_f64(state[e][R.MT_N + 2:])[0]))
        else:
            assert state[e][R.MT_N + 2] == want[R.MT_N + 2]
    finish(t, "MT19937", what)
    return replays


def test_seeding_matches_numpy_for_one_and_two_digit_keys(probe):
    C.test_seeding_matches_numpy_for_one_and_two_digit_keys(probe)


def test_per_env_mt19937_is_numpys_stream(probe):
    keys, lens, skip, stride = C.per_env_case()
    check_mt_device(probe, R.GEN_MT, R.per_env_program(), keys, lens, skip, stride, "Mt19937, 70 envs", min_words=1900, min_twists=3)


def test_masked_envs_never_draw(probe):
    C.test_per_env_mt19937_masked_envs_never_draw(probe)       # (programs without a Gaussian draw: everything exact)
    C.test_group_mt_masked_env_never_draws(probe)


def test_group_mt_is_numpys_stream_for_every_window_phase(probe):
    keys, lens, skip, stride = C.group_mt_case()
    rps = check_mt_device(probe, R.GEN_GROUP_MT, R.group_mt_program(), keys, lens, skip, stride, "GroupMt, 6 envs", min_words=1900, min_twists=3)
    short = set()
    for rp in rps:
        short |= {c for c in rp.refills if c < R.GL}
    assert short == set(range(1, R.GL)), sorted(short)


def test_lane0_mt19937_is_numpys_stream(probe):
    keys, lens = R.seed_keys([0, 1, 12345, 2 ** 40 + 7, 2 ** 32 - 1, 2 ** 32])
    check_mt_device(probe, R.GEN_LANE0_MT, R.lane0_program(), keys, lens, 560 + 13 * np.arange(6), 32, "Lane0Rng<Mt19937>, 6 envs", min_twists=2)


def test_handover_between_the_forms_is_one_numpy_stream(probe):
    keys, lens = R.seed_keys([3, 2 ** 40 + 7, 99])
    outs_v, state = C.run_handover(probe, keys, lens, 29)
    outs_z, state_z = C.run_handover(probe, keys, lens, 29, std_normals=True)
    assert np.array_equal(state, state_z)
    t = R.GaussTally()
    for e in range(len(keys)):
        rp = R.MtReplay(R.key_list(keys, lens, e))
        for (gen, program), v, z in zip(R.handover_programs(), outs_v, outs_z):
            C.assert_lanes_agree(v)
            C.assert_lanes_agree(z)
            first, first_g = len(rp.values), len(rp.gauss)
            rp.run(program)
            stage = R.MtReplay.__new__(R.MtReplay)             # this stage's slice of the one stream
            stage.values = rp.values[first:]
            stage.gauss = [(g[0] - first,) + tuple(g[1:]) for g in rp.gauss[first_g:]]
            exact_but_gaussians(gen, program, v[e:e + 1], [stage])
            hold_gaussians(t, R.mt_deviate_exact, [stage], z[e:e + 1], v[e:e + 1])
        assert np.array_equal(state[e][:R.MT_N + 2], rp.state_row()[:R.MT_N + 2]), e
    finish(t, "MT19937", "hand-over Mt19937 / GroupMt / Lane0Rng on one state, 3 envs")


def check_philox_device(probe, gen, stream, program, ctr0, what):
    keys = R.philox_keys()
    c0 = np.array(ctr0, np.uint64)
    v, state = R.run(probe, gen, program, keys, skip=R.PHILOX_SKIP, stream=stream, state_in=c0)
    z, _ = R.run(probe, gen, program, keys, skip=R.PHILOX_SKIP, stream=stream, state_in=c0, std_normals=True)
    C.assert_lanes_agree(v)
    C.assert_lanes_agree(z)
    replays = []
    for e in range(len(keys)):
        rp = R.PhiloxReplay(keys[e][0], keys[e][1], ctr0[e], stream)
        rp.skip(R.PHILOX_SKIP[e])
        rp.run(program)
        assert int(state[e][0]) == rp.ctr, (R.GEN_NAMES[gen], "counter of env", e)
        replays.append(rp)
    exact_but_gaussians(gen, program, v, replays)
    exact_but_gaussians(gen, program, z, replays)
    t = R.GaussTally()
    hold_gaussians(t, R.philox_deviate_exact, replays, z, v)
    finish(t, "Philox", what)
    return v, z


@pytest.mark.parametrize("ctr0", sorted(R.PHILOX_CTR0))
def test_philox_family_is_the_sequential_stream(probe, ctr0):
    c0 = R.PHILOX_CTR0[ctr0]
    for stream in (0, 1):
        check_philox_device(probe, R.GEN_PHILOX, stream, [(R.U32, (), 3)] + R.philox_program(), c0, "Philox stream {} ({})".format(stream, ctr0))
    lane = check_philox_device(probe, R.GEN_PHILOX, 0, R.philox_program(), c0, "Philox ({})".format(ctr0))
    group = check_philox_device(probe, R.GEN_GROUP_PHILOX, 0, R.philox_program(), c0, "GroupPhilox ({})".format(ctr0))
    for g, l in zip(group, lane):                              # Gaussian values included: one device code for both forms
        assert np.array_equal(g[:, 0], l[:, 0])
    lane, _ = C.check_philox(probe, R.GEN_PHILOX, 1, R.actions_program(), c0, R.PHILOX_SKIP)          # (no Gaussian draw: all exact)
    group, _ = C.check_philox(probe, R.GEN_GROUP_ACTIONS, 1, R.actions_program(), c0, R.PHILOX_SKIP)
    assert np.array_equal(group[:, 0], lane[:, 0])


def test_probe_refuses_what_a_form_cannot_run(probe):
    C.test_probe_refuses_what_a_form_cannot_run(probe)


def test_zz_gaussian_totals_of_this_file():
    """Last in the file: the totals over every Gaussian deviate drawn above, printed; each deviate was already held to its bound."""
    for name, t in sorted(TALLY.items()):
        print(t.line("TOTAL " + name + " on the device"))
        assert t.n > 0 and t.got_worst <= t.ref_worst + 1.0
    assert TALLY["MT19937"].n + TALLY["Philox"].n <= 20000
