"""The random generators of the kernels (csrc/rng.hpp: Mt19937, Philox; csrc/kuka_group.hpp: GroupMt, Lane0Rng, GroupPhilox,
GroupActions) compiled for the host (hostcheck_rng_probe: the interpreter of csrc/rng_probe.hpp, the 16 lanes of a group as
lockstep fibers), word for word against numpy's RandomState and the Philox4x32-10 definition.  Host code calls libm, so here
EVERYTHING — Gaussian values included — equals numpy (MT19937) or oracle/philox.h (Philox) bit for bit.  The same programs and the
same replays run on the device in tests/test_gpu_rng_streams.py; this file is what checks them without a GPU."""
import numpy as np
import pytest

import rng_stream_ref as R


@pytest.fixture(scope="module")
def probe():
    return R.host_probe()


def assert_lanes_agree(out):
    assert np.array_equal(out, np.broadcast_to(out[:, :1, :], out.shape)), "the lanes of an env saw different values"


def check_mt(probe, gen, program, keys, lens, skip, stride, min_words=0, min_twists=0, mask=None):
    """Runs `program` on an MT form and holds values, words consumed and the persisted state to numpy.  -> the replays"""
    out, state = R.run(probe, gen, program, keys, lens, skip=skip, stride=stride, mask=mask)
    assert_lanes_agree(out)
    replays = []
    for e in range(len(keys)):
        rp = R.MtReplay(R.key_list(keys, lens, e))
        if mask is not None and not mask[e]:                   # never drew: the state as seeded, nothing written
            assert not out[e].any() and np.array_equal(state[e], rp.state_row()), e
            replays.append(None)
            continue
        rp.skip(int(skip[e]))
        rp.run(program)
        got, want = out[e, 0], np.array(rp.values, dtype=np.uint64)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (R.GEN_NAMES[gen], "env", e, "first differing value", int(bad[0]), R.value_ops(gen, program)[bad[0]])
        assert np.array_equal(state[e], rp.state_row()), (R.GEN_NAMES[gen], "state of env", e, int(state[e][R.MT_N]), rp.rs.get_state()[2])
        assert rp.words >= min_words and rp.twists >= min_twists, (e, rp.words, rp.twists)
        replays.append(rp)
    return replays


def test_philox_definition_reproduces_the_published_vectors():
    for ctr, key, want in R.PHILOX_KAT:
        assert R.philox4x32_10(ctr, key) == want


def test_seeding_matches_numpy_for_one_and_two_digit_keys(probe):
    keys, lens = R.seeding_keys()
    assert set(lens.tolist()) == {1, 2}
    _, state = R.run(probe, R.GEN_MT, [], keys, lens, stride=len(keys) + 26)
    for e in range(len(keys)):
        rs = np.random.RandomState()
        rs.seed(R.key_list(keys, lens, e))
        assert np.array_equal(state[e], R.np_state_row(rs)), (e, R.key_list(keys, lens, e))
        assert state[e][R.MT_N] == R.MT_N and state[e][R.MT_N + 1] == 0


def per_env_case():
    n = 70
    keys, lens = R.seed_keys(np.arange(n))
    keys[68], lens[68] = (12345, 0), 1                         # one-digit keys among them
    keys[69], lens[69] = (R.M32, 0), 1
    return keys, lens, np.arange(n), 96


def test_per_env_mt19937_is_numpys_stream(probe):
    keys, lens, skip, stride = per_env_case()
    check_mt(probe, R.GEN_MT, R.per_env_program(), keys, lens, skip, stride, min_words=1900, min_twists=3)


def test_per_env_mt19937_masked_envs_never_draw(probe):
    keys, lens, skip, stride = per_env_case()
    mask = (np.arange(len(keys)) % 3 != 1).astype(np.uint8)
    check_mt(probe, R.GEN_MT, R.per_env_program()[:6], keys[:9], lens[:9], skip[:9], 13, mask=mask[:9])


def group_mt_case():
    keys, lens = R.seed_keys([0, 1, 12345, 2 ** 40 + 7, 2 ** 32 - 1, 2 ** 32])
    return keys, lens, np.arange(6) + 1, 32


def test_group_mt_is_numpys_stream_for_every_window_phase(probe):
    keys, lens, skip, stride = group_mt_case()
    rps = check_mt(probe, R.GEN_GROUP_MT, R.group_mt_program(), keys, lens, skip, stride, min_words=1900, min_twists=3)
    short = set()
    for rp in rps:
        short |= {c for c in rp.refills if c < R.GL}
    assert short == set(range(1, R.GL)), sorted(short)         # every cnt < 16 window right in front of a twist


def test_group_mt_masked_env_never_draws(probe):
    keys, lens, skip, stride = group_mt_case()
    check_mt(probe, R.GEN_GROUP_MT, R.group_mt_program()[:8], keys, lens, skip, stride, mask=np.array([1, 0, 1, 1, 0, 1], np.uint8))


def test_lane0_mt19937_is_numpys_stream(probe):
    keys, lens = R.seed_keys([0, 1, 12345, 2 ** 40 + 7, 2 ** 32 - 1, 2 ** 32])
    check_mt(probe, R.GEN_LANE0_MT, R.lane0_program(), keys, lens, 560 + 13 * np.arange(6), 32, min_twists=2)


def run_handover(probe, keys, lens, stride, std_normals=False):
    """the stages of R.handover_programs() one after the other on one state -> (per stage out, final state)"""
    outs, state = [], None
    for gen, program in R.handover_programs():
        out, state = R.run(probe, gen, program, keys, lens, stride=stride, state_in=state, std_normals=std_normals)
        outs.append(out)
    return outs, state


def test_handover_between_the_forms_is_one_numpy_stream(probe):
    keys, lens = R.seed_keys([3, 2 ** 40 + 7, 99])
    outs, state = run_handover(probe, keys, lens, 29)
    for e in range(len(keys)):
        rp = R.MtReplay(R.key_list(keys, lens, e))
        for (gen, program), out in zip(R.handover_programs(), outs):
            assert_lanes_agree(out)
            first = len(rp.values)
            rp.run(program)
            assert np.array_equal(out[e, 0], np.array(rp.values[first:], dtype=np.uint64)), (e, R.GEN_NAMES[gen])
        assert np.array_equal(state[e], rp.state_row()), e


def check_philox(probe, gen, stream, program, ctr0, skip):
    keys = R.philox_keys()
    out, state = R.run(probe, gen, program, keys, skip=skip, stream=stream, state_in=np.array(ctr0, np.uint64))
    assert_lanes_agree(out)
    replays = []
    for e in range(len(keys)):
        rp = R.PhiloxReplay(keys[e][0], keys[e][1], ctr0[e], stream)
        rp.skip(int(skip[e]))
        rp.run(program)
        got, want = out[e, 0], np.array(rp.values, dtype=np.uint64)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (R.GEN_NAMES[gen], "env", e, "first differing value", int(bad[0]), R.value_ops(gen, program)[bad[0]])
        assert int(state[e][0]) == rp.ctr, (R.GEN_NAMES[gen], "counter of env", e)
        replays.append(rp)
    return out, replays


@pytest.mark.parametrize("ctr0", sorted(R.PHILOX_CTR0))
def test_philox_family_is_the_sequential_stream(probe, ctr0):
    c0 = R.PHILOX_CTR0[ctr0]
    for stream in (0, 1):
        check_philox(probe, R.GEN_PHILOX, stream, [(R.U32, (), 3)] + R.philox_program(), c0, R.PHILOX_SKIP)
    lane, _ = check_philox(probe, R.GEN_PHILOX, 0, R.philox_program(), c0, R.PHILOX_SKIP)
    group, _ = check_philox(probe, R.GEN_GROUP_PHILOX, 0, R.philox_program(), c0, R.PHILOX_SKIP)
    assert np.array_equal(group[:, 0], lane[:, 0])             # the batched form against the per-lane one, same key and counter
    lane, _ = check_philox(probe, R.GEN_PHILOX, 1, R.actions_program(), c0, R.PHILOX_SKIP)
    group, _ = check_philox(probe, R.GEN_GROUP_ACTIONS, 1, R.actions_program(), c0, R.PHILOX_SKIP)
    assert np.array_equal(group[:, 0], lane[:, 0])


def test_probe_refuses_what_a_form_cannot_run(probe):
    keys = R.philox_keys()
    n = len(keys)
    out, state = np.zeros(64, np.uint64), np.zeros(n * R.MT_STATE, np.uint64)
    skip, lens = np.zeros(n, np.int32), np.full(n, 2, np.int32)
    keys_t = np.ascontiguousarray(keys.T)

    def call(gen, program, out_words=out.size, stride=n):
        script, args = R.compile_program(program)
        return probe(0, gen, 0, n, stride, R._p(keys_t), R._p(lens), None, None, R._p(script), len(script), R._p(args), len(args) - 1,
                     R._p(skip), R._p(out), out_words, R._p(state), state.size)
    assert call(R.GEN_GROUP_ACTIONS, [(R.NORMAL, (0.0, 1.0), 1)]) == -22
    assert call(R.GEN_GROUP_PHILOX, [(R.U32, (), 1)]) == -22
    assert call(R.GEN_MT, [(R.SET_CTR, (1,), 1)]) == -22
    assert call(R.GEN_MT, [(R.BOUNDED, (2.0 ** 32,), 1)]) == -22
    assert call(R.GEN_MT, [(R.U32, (), 4)], out_words=n * 4 - 1) == -22          # out too small for the script
    assert call(R.GEN_MT, [(R.U32, (), 1)], stride=n - 1) == -22
    assert call(R.GEN_MT, [(R.U32, (), 1)]) == 0


def test_gaussian_values_equal_the_reference_and_stay_inside_its_bound(probe):
    """The ulp machinery of the GPU test on host values: the reference's worst error against the 200-bit value, the probed
    generator's (equal bits here, so equal errors), and loc + scale z as the unfused double result."""
    keys, lens = R.seed_keys([0, 1, 12345])
    program = [(R.U32, (), 1), (R.NORMAL, (7.0, 1.0), 5), (R.STORE_LOAD, (), 1), (R.NORMAL, (0.5, 0.01), 40)]
    tally = R.GaussTally()
    for gen in (R.GEN_MT, R.GEN_GROUP_MT):
        z, _ = R.run(probe, gen, program, keys, lens, stride=7, std_normals=True)
        v, _ = R.run(probe, gen, program, keys, lens, stride=7)
        for e in range(len(keys)):
            rp = R.MtReplay(R.key_list(keys, lens, e)).run(program)
            R.check_gaussians(rp, R.mt_deviate_exact, z[e, 0], v[e, 0], tally)
    print(tally.line("MT19937 forms on the host"))
    assert tally.mismatch == 0 and tally.got_worst <= tally.ref_worst + 1.0
    tally = R.GaussTally()
    c0 = R.PHILOX_CTR0["staggered"]
    for gen in (R.GEN_PHILOX, R.GEN_GROUP_PHILOX):
        z, _ = R.run(probe, gen, R.philox_program(), R.philox_keys(), skip=R.PHILOX_SKIP, state_in=np.array(c0, np.uint64), std_normals=True)
        v, _ = R.run(probe, gen, R.philox_program(), R.philox_keys(), skip=R.PHILOX_SKIP, state_in=np.array(c0, np.uint64))
        for e in range(6):
            rp = R.PhiloxReplay(R.philox_keys()[e][0], R.philox_keys()[e][1], c0[e], 0)
            rp.skip(R.PHILOX_SKIP[e])
            rp.run(R.philox_program())
            R.check_gaussians(rp, R.philox_deviate_exact, z[e, 0], v[e, 0], tally)
    print(tally.line("Philox forms on the host"))
    assert tally.mismatch == 0 and tally.got_worst <= tally.ref_worst + 1.0
