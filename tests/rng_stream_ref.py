"""Shared by tests/test_rng_streams_cpu.py and tests/test_gpu_rng_streams.py: the scripted draw programs run through the generator
self-test (csrc/rng_probe.hpp: srlhip_selftest_rng on the device, hostcheck_rng_probe on the host), and their references written
from the definitions — numpy's RandomState itself for the MT19937 forms, a plain-integer Philox4x32-10 for the Philox family, mpmath
for the value of a Gaussian deviate."""
import ctypes
import functools
import math

import numpy as np

from oracle import clib, gym_seeding

GEN_MT, GEN_GROUP_MT, GEN_LANE0_MT, GEN_PHILOX, GEN_GROUP_PHILOX, GEN_GROUP_ACTIONS = range(6)
GEN_NAMES = ("Mt19937", "GroupMt", "Lane0Rng<Mt19937>", "Philox", "GroupPhilox", "GroupActions")
U32, DOUBLE01, UNIFORM, NORMAL, BOUNDED, STORE_LOAD, SET_CTR = range(7)
MT_N = 624
MT_STATE = MT_N + 3
GL = 16
# bounded(r): the mask edges and the rejection-free extremes
BOUNDED_EDGES = (0, 1, 2, 5, 6, 255, 256, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1)


def is_mt(gen):
    return gen in (GEN_MT, GEN_GROUP_MT, GEN_LANE0_MT)


def lanes_of(gen):
    return 1 if gen in (GEN_MT, GEN_PHILOX) else GL


# ---------------------------------------------------------------------------------------------------------------- programs
# A program is a list of (op, params, repeat); params: () | (lo, hi) | (loc, scale) | (r,) | (offset,).
def compile_program(program, std_normals=False):
    """-> (script int32 [n_ops][3], args float64); std_normals: every normal draws (0, 1), i.e. the deviate itself"""
    script, args = [], []
    for op, params, rep in program:
        if op == NORMAL and std_normals:
            params = (0.0, 1.0)
        script.append((op, len(args), rep))
        args.extend(float(p) for p in params)
    return (np.asarray(script, dtype=np.int32).reshape(-1, 3), np.asarray(args + [0.0], dtype=np.float64))


def values_of(gen, program):
    return sum(rep * (4 if (op == U32 and gen == GEN_PHILOX) else 1) for op, _, rep in program if op < STORE_LOAD)


def value_ops(gen, program):
    """per output value: (op, params)"""
    out = []
    for op, params, rep in program:
        if op < STORE_LOAD:
            out.extend([(op, params)] * (rep * (4 if (op == U32 and gen == GEN_PHILOX) else 1)))
    return out


_PROBE_ARGTYPES = [ctypes.c_int32] * 5 + [ctypes.c_void_p] * 5 + [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                                                  ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]


def host_probe():
    import hostcheck
    fn = hostcheck.lib().hostcheck_rng_probe
    fn.argtypes = _PROBE_ARGTYPES
    return fn


def device_probe():
    from srlhip import _lib
    return _lib.load().srlhip_selftest_rng


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def run(fn, gen, program, keys, key_len=None, skip=None, stride=0, stream=0, mask=None, state_in=None, std_normals=False):
    """One probe call.  keys: [n][2] uint32.  -> (out uint64 [n][lanes][values], state uint64 [n][627 | 1])"""
    keys = np.asarray(keys, dtype=np.uint32).reshape(-1, 2)
    n = len(keys)
    keys_t = np.ascontiguousarray(keys.T)                      # [2][n]
    key_len = None if key_len is None else np.ascontiguousarray(key_len, dtype=np.int32)
    skip = np.zeros(n, np.int32) if skip is None else np.ascontiguousarray(skip, dtype=np.int32)
    mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    state_in = None if state_in is None else np.ascontiguousarray(state_in, dtype=np.uint64)
    script, args = compile_program(program, std_normals)
    lanes, values = lanes_of(gen), values_of(gen, program)
    out = np.full((n, lanes, values), 0xDEADBEEF, dtype=np.uint64)
    state = np.zeros((n, MT_STATE if is_mt(gen) else 1), dtype=np.uint64)
    rc = fn(0, gen, stream, n, stride, _p(keys_t), _p(key_len), _p(mask), _p(state_in), _p(script), len(script), _p(args), len(args) - 1,
            _p(skip), _p(out), out.size, _p(state), state.size)
    assert rc == 0, (GEN_NAMES[gen], rc)
    return out, state


def seed_keys(seeds):
    """gym's key digits of each seed -> (keys [n][2], key_len [n])"""
    return clib.mt_keys(seeds)


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def as_f64(u):
    return np.asarray(u, dtype=np.uint64).view(np.float64)


# ------------------------------------------------------------------------------------------------------------ MT19937: numpy
def np_state_row(rs):
    _, words, pos, has, g = rs.get_state()
    return np.concatenate([words.astype(np.uint64), np.array([pos, has], np.uint64), bits([g])])


def np_from_row(row):
    rs = np.random.RandomState()
    rs.set_state(("MT19937", np.asarray(row[:MT_N], dtype=np.uint32), int(row[MT_N]), int(row[MT_N + 1]), float(as_f64(row[MT_N + 2:MT_N + 3])[0])))
    return rs


def _clone(rs):
    c = np.random.RandomState()
    c.set_state(rs.get_state())
    return c


class MtReplay(object):
    """numpy's RandomState replaying a program: values (uint64 bits), the state row, the words consumed, and per Gaussian draw what
    stands in front of the transcendental functions (the factor x and r2 of the accepted pair: exact double arithmetic).  The window
    bookkeeping (refills) models only WHEN GroupMt fetches words — for the tests' coverage assertions, never for an expected value."""

    def __init__(self, key=None, state_row=None):
        if state_row is not None:
            self.rs = np_from_row(state_row)
        else:
            self.rs = np.random.RandomState()
            self.rs.seed([int(k) for k in key])
        self.values, self.gauss = [], []      # gauss: (value index, x, r2, numpy's deviate, loc, scale)
        self.words = 0
        self.twists = 0
        self.refills = []                     # 624 - idx at every window refill of a 16-word window reader
        self._win = 0
        self._pos = self.rs.get_state()[2]
        self._pending = None                  # (x1, r2) of the cached deviate

    def _consume(self, k):
        """k words drawn one after the other, starting at index self._pos"""
        for _ in range(k):
            if self._win == 0:
                if self._pos == MT_N:
                    self._pos = 0
                    self.twists += 1
                self.refills.append(MT_N - self._pos)
                self._win = min(GL, MT_N - self._pos)
            self._win -= 1
            self._pos += 1
        self.words += k

    def _delta(self, before):
        after = self.rs.get_state()[2]
        return (after - before) % MT_N if after != before else 0

    def skip(self, k):
        if k:
            self.rs.randint(0, 2 ** 32, size=k, dtype=np.uint64)
            self._consume(k)

    def run(self, program):
        rs = self.rs
        for op, params, rep in program:
            if op == U32:
                self.values.extend(int(v) for v in rs.randint(0, 2 ** 32, size=rep, dtype=np.uint64))
                self._consume(rep)
            elif op == DOUBLE01:
                self.values.extend(int(v) for v in bits(rs.random_sample(rep)))
                self._consume(2 * rep)
            elif op == UNIFORM:
                self.values.extend(int(v) for v in bits(rs.uniform(params[0], params[1], size=rep)))
                self._consume(2 * rep)
            elif op == BOUNDED:
                for _ in range(rep):
                    before = rs.get_state()[2]
                    self.values.append(int(rs.randint(0, int(params[0]) + 1)))
                    self._consume(self._delta(before) if params[0] else 0)
            elif op == NORMAL:
                for _ in range(rep):
                    _, _, before, has, _ = rs.get_state()
                    z = float(_clone(rs).standard_normal())
                    if has:
                        x, r2 = self._pending
                        self._pending = None
                    else:                     # the polar method's accepted pair, in the exact double arithmetic of the definition
                        c = _clone(rs)
                        while True:
                            x1 = 2.0 * c.random_sample() - 1.0
                            x2 = 2.0 * c.random_sample() - 1.0
                            r2 = x1 * x1 + x2 * x2
                            if not (r2 >= 1.0 or r2 == 0.0):
                                break
                        x, self._pending = x2, (x1, r2)
                    v = float(rs.normal(params[0], params[1]))
                    self.gauss.append((len(self.values), x, r2, z, float(params[0]), float(params[1])))
                    self.values.append(int(bits([v])[0]))
                    self._consume(self._delta(before) if not has else 0)
            elif op == STORE_LOAD:
                self._win = 0                 # a window reader drops what it had fetched
            else:
                raise ValueError(op)
        return self

    def state_row(self):
        return np_state_row(self.rs)


# ------------------------------------------------------------------------------------------------- Philox4x32-10: the definition
M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Random123's philox4x32-10: counter (4 words), key (2 words) -> 4 words"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return (c0, c1, c2, c3)


# the known-answer vectors of the Random123 distribution (kat_vectors: philox4x32 10)
PHILOX_KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def project_block(k0, k1, ctr, stream):
    """the project's counter layout on top: (ctr lo, ctr hi, stream, 0x5eed5eed)"""
    return philox4x32_10((ctr & M32, (ctr >> 32) & M32, stream, 0x5eed5eed), (k0, k1))


def to_double(a, b):
    return ((a >> 5) * 67108864.0 + (b >> 6)) / 9007199254740992.0


TWO_PI = 6.283185307179586476925286766559      # (rounds to the double the kernels' literal rounds to)


def oracle_philox(k0, k1, ctr, stream):
    """oracle/philox.h at one counter -> (words, double01, std_normal through libm)"""
    w, u, g = np.zeros(4, np.uint32), np.zeros(1), np.zeros(1)
    fn = clib.lib().oracle_philox_draws
    fn.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    fn.restype = None
    fn(k0, k1, ctr & (2 ** 64 - 1), stream, 1, _p(w), _p(u), _p(g))
    return tuple(int(x) for x in w), float(u[0]), float(g[0])


class PhiloxReplay(object):
    """The sequential Philox stream of one env from the definition: values, the counter, and per Gaussian draw (value index, u1,
    the rounded product 2 pi u2, the oracle's deviate, loc, scale).  group: skip draws are whole draws of the group forms."""

    def __init__(self, k0, k1, ctr0, stream):
        self.k0, self.k1, self.ctr0, self.ctr, self.stream = int(k0), int(k1), int(ctr0), int(ctr0), int(stream)
        self.values, self.gauss = [], []

    def _block(self):
        w = project_block(self.k0, self.k1, self.ctr, self.stream)
        ow, _, _ = oracle_philox(self.k0, self.k1, self.ctr, self.stream)
        assert w == ow, "oracle/philox.h and the definition disagree at counter {}".format(self.ctr)
        self.ctr = (self.ctr + 1) & (2 ** 64 - 1)
        return w

    def skip(self, k):
        self.ctr = (self.ctr + k) & (2 ** 64 - 1)

    def run(self, program):
        for op, params, rep in program:
            for _ in range(rep):
                if op == U32:
                    self.values.extend(self._block())
                elif op == DOUBLE01:
                    w = self._block()
                    self.values.append(int(bits([to_double(w[0], w[1])])[0]))
                elif op == UNIFORM:
                    w = self._block()
                    lo, hi = float(params[0]), float(params[1])
                    self.values.append(int(bits([lo + (hi - lo) * to_double(w[0], w[1])])[0]))
                elif op == BOUNDED:
                    w = self._block()
                    self.values.append((w[0] * (int(params[0]) + 1)) >> 32)
                elif op == NORMAL:
                    _, _, z = oracle_philox(self.k0, self.k1, self.ctr, self.stream)
                    w = self._block()
                    u1, u2 = 1.0 - to_double(w[0], w[1]), to_double(w[2], w[3])
                    loc, scale = float(params[0]), float(params[1])
                    self.gauss.append((len(self.values), u1, TWO_PI * u2, z, loc, scale))
                    self.values.append(int(bits([loc + scale * z])[0]))
                elif op == SET_CTR:
                    self.ctr = (self.ctr0 + int(params[0])) & (2 ** 64 - 1)
                elif op != STORE_LOAD:
                    raise ValueError(op)
        return self


# -------------------------------------------------------------------------------------------------- Gaussian values: mpmath
def _mp():
    import mpmath
    mpmath.mp.prec = 200
    return mpmath


def ulp_error(got, exact):
    """|got - exact| in units of the spacing of doubles at exact (exact: mpf)"""
    mp = _mp()
    if exact == 0:
        return 0.0 if got == 0.0 else float("inf")
    e = math.frexp(float(exact))[1]                     # |exact| in [2^(e-1), 2^e)
    return float(abs(mp.mpf(got) - exact) / mp.ldexp(mp.mpf(1), e - 53))


@functools.lru_cache(maxsize=None)
def mt_deviate_exact(x, r2):
    """sqrt(-2 log(r2) / r2) x at 200 bits, from the doubles x and r2"""
    mp = _mp()
    r = mp.mpf(r2)
    return mp.sqrt(-2 * mp.log(r) / r) * mp.mpf(x)


@functools.lru_cache(maxsize=None)
def philox_deviate_exact(u1, arg):
    """sqrt(-2 log(u1)) cos(arg) at 200 bits, from the doubles u1 and arg = fl(2 pi u2)"""
    mp = _mp()
    return mp.sqrt(-2 * mp.log(mp.mpf(u1))) * mp.cos(mp.mpf(arg))


class GaussTally(object):
    """Over the Gaussian draws of a test file: the reference's own worst error against the 200-bit value, the probed generator's,
    and how many of its deviates differ from the reference's bit for bit."""

    def __init__(self):
        self.n = self.mismatch = 0
        self.ref_worst = self.got_worst = 0.0

    def add(self, exact, ref_z, got_z):
        self.n += 1
        self.ref_worst = max(self.ref_worst, ulp_error(ref_z, exact))
        self.got_worst = max(self.got_worst, ulp_error(got_z, exact))
        self.mismatch += int(bits([ref_z])[0] != bits([got_z])[0])

    def merge(self, other):
        self.n += other.n
        self.mismatch += other.mismatch
        self.ref_worst, self.got_worst = max(self.ref_worst, other.ref_worst), max(self.got_worst, other.got_worst)

    def line(self, what):
        return "{}: {} deviates, {} differ from the reference's bits ({:.3%}); worst error vs 200-bit value: reference {:.3f} ulp, probed {:.3f} ulp".format(
            what, self.n, self.mismatch, self.mismatch / max(1, self.n), self.ref_worst, self.got_worst)


def check_gaussians(replay, exact_fn, z_got, v_got, tally):
    """One env's Gaussian draws.  z_got / v_got: the probed values (uint64 bits, indexed like replay.values) of the run with every
    normal as (0, 1) and of the run with the program's own (loc, scale).  Holds loc + scale z to the unfused double result of the
    probed generator's own z, exactly; adds every deviate to the tally."""
    for k, a, b, z_ref, loc, scale in replay.gauss:
        z = float(as_f64([z_got[k]])[0])
        v = float(as_f64([v_got[k]])[0])
        want = loc + scale * z                                   # two roundings: numpy's unfused order
        assert bits([v])[0] == bits([want])[0], ("loc + scale * z is not the unfused double result", k, loc, scale, z, v, want)
        tally.add(exact_fn(a, b), z_ref, z)


# -------------------------------------------------------------------------------------------------------------- the scripts
SEEDS_SIX = (0, 1, 12345, 2 ** 40 + 7, 2 ** 32 - 1, 2 ** 32)
# gym's hash spreads every seed over 64 bits, so its keys have two digits but for one seed in 2^32: one-digit keys are given directly
RAW_KEYS = (((12345, 0), 1), ((0, 0), 1), ((M32, 0), 1), ((1, 0), 2), ((0, 0), 2), ((M32, M32), 2))


def seeding_keys():
    keys, lens = seed_keys(SEEDS_SIX)
    keys = np.concatenate([keys, np.array([k for k, _ in RAW_KEYS], np.uint32)])
    lens = np.concatenate([lens, np.array([l for _, l in RAW_KEYS], np.int32)])
    return keys, lens


def key_list(keys, lens, e):
    return [int(k) for k in keys[e][:lens[e]]]


def per_env_program():
    p = [(U32, (), 300), (DOUBLE01, (), 100), (UNIFORM, (-0.3, 1.7), 50)]
    p += [(BOUNDED, (r,), 8) for r in BOUNDED_EDGES]
    p += [(NORMAL, (7.0, 1.0), 5), (STORE_LOAD, (), 1), (NORMAL, (0.0, 0.25), 4), (STORE_LOAD, (), 1), (U32, (), 3), (NORMAL, (-2.0, 3.0), 2)]
    p += [(U32, (), 900), (NORMAL, (0.5, 2.0), 11), (STORE_LOAD, (), 1), (DOUBLE01, (), 200)]
    p += [(BOUNDED, (5,), 20), (BOUNDED, (2 ** 31,), 10), (NORMAL, (0.0, 1.0), 7), (U32, (), 2)]
    return p


def group_mt_program():
    # three window phases per env: a load at index i, then 629 words across the twist (the next load stands 5 words further in its window)
    p = []
    for _ in range(3):
        p += [(STORE_LOAD, (), 1), (U32, (), 629)]
    # the env's own pattern: reset draws, then one noise draw per step; the cached deviate and a half-used window cross a store + load
    p += [(NORMAL, (7.0, 1.0), 5), (STORE_LOAD, (), 1), (UNIFORM, (-0.1, 0.1), 3), (BOUNDED, (2,), 2)]
    for t in range(300):
        p.append((NORMAL, (0.0, 0.01), 1))
        if t % 7 == 3:
            p.append((UNIFORM, (-0.1, 0.1), 1))
        if t == 150:
            p.append((STORE_LOAD, (), 1))
    p += [(BOUNDED, (r,), 3) for r in BOUNDED_EDGES]
    p += [(DOUBLE01, (), 9), (U32, (), 5)]
    return p


def lane0_program():
    p = [(DOUBLE01, (), 5), (UNIFORM, (2.0, 3.0), 5), (NORMAL, (7.0, 1.0), 5), (STORE_LOAD, (), 1), (NORMAL, (0.0, 0.01), 4)]
    p += [(BOUNDED, (r,), 3) for r in BOUNDED_EDGES]
    p += [(NORMAL, (-1.0, 0.5), 3), (STORE_LOAD, (), 1), (DOUBLE01, (), 40), (NORMAL, (0.0, 1.0), 2)]
    return p


def handover_programs():
    """(generator, program) stages run one after the other on ONE state; numpy replays their concatenation as one stream"""
    return [
        (GEN_MT, [(U32, (), 10), (NORMAL, (1.0, 2.0), 3)]),                       # odd: has_gauss is set at the hand-over
        (GEN_GROUP_MT, [(NORMAL, (0.0, 1.0), 4), (U32, (), 650), (NORMAL, (7.0, 1.0), 1)]),
        (GEN_MT, [(NORMAL, (0.0, 0.5), 2), (DOUBLE01, (), 3)]),
        (GEN_LANE0_MT, [(NORMAL, (0.0, 1.0), 2), (UNIFORM, (0.0, 2.0), 3), (BOUNDED, (5,), 4)]),
        (GEN_GROUP_MT, [(DOUBLE01, (), 7), (NORMAL, (3.0, 0.1), 3)]),
        (GEN_MT, [(NORMAL, (0.0, 1.0), 1), (U32, (), 4)]),
    ]


PHILOX_SEEDS = (0, 1, 12345, 2 ** 40 + 7, 2 ** 32 - 1, 2 ** 63 - 1)
PHILOX_CTR0 = {
    "staggered": [5 * e for e in range(6)],
    "carry": [0, 5, 2 ** 32 - 8, 15, 20, 25],          # env 2: its first batch straddles the carry into the counter's high word
}
PHILOX_SKIP = [0, 3, 6, 9, 12, 15]                     # group forms: where each row stands in its batch when the script starts


def philox_keys():
    return np.array([(s & M32, s >> 32) for s in PHILOX_SEEDS], np.uint32)


def philox_program():
    return [
        (NORMAL, (7.0, 1.0), 3), (DOUBLE01, (), 2), (NORMAL, (0.0, 0.01), 5), (BOUNDED, (5,), 1), (NORMAL, (0.0, 1.0), 9),
        (UNIFORM, (-1.0, 1.0), 2), (BOUNDED, (0,), 1), (BOUNDED, (2 ** 32 - 1,), 2), (NORMAL, (-3.0, 2.0), 4),
        (SET_CTR, (1000,), 1), (NORMAL, (0.0, 1.0), 16), (NORMAL, (1.0, 1.0), 1),          # exactly one batch from a fresh base, then the refill
        (STORE_LOAD, (), 1), (NORMAL, (0.0, 0.5), 3), (DOUBLE01, (), 1), (NORMAL, (0.0, 1.0), 20),
    ]


def actions_program():
    # GroupActions fills a batch with ONE bound (the kernels only ever ask for bounded(5)): a new bound starts from a fresh base.
    # next() returns an int (an action), so the largest bound whose draws it can return is 2^31 - 1; the per-lane Philox and
    # GroupPhilox run bounded(2^32 - 1) in philox_program().
    return [
        (BOUNDED, (5,), 20), (SET_CTR, (40,), 1), (BOUNDED, (0,), 3), (SET_CTR, (50,), 1), (BOUNDED, (2 ** 31 - 1,), 17),
        (SET_CTR, (77,), 1), (BOUNDED, (5,), 16), (BOUNDED, (5,), 1), (STORE_LOAD, (), 1), (BOUNDED, (5,), 5),
    ]
