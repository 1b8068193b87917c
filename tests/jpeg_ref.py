"""The arithmetic contract of srlhip_jpeg_encode (include/srlhip.h) restated in numpy: encode(frame_hw3, quality) -> bytes.
A test helper like tests/policy_exact.py.  Tables and header are written from the JPEG specification (ITU-T T.81: Annex K.1 - K.3,
Figure A.6, Annex B for the segments, Annex C for the code assignment, F.1.2 for the coding) and from the contract — nothing here is
read from the product.  `stats`, when given, collects what the tests' preconditions ask about the stream."""
import numpy as np

HEADER_BYTES = 629

K1 = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
K2 = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def _zigzag():
    """Figure A.6, generated: walk the anti-diagonals, alternating direction"""
    order = []
    for d in range(15):
        cells = [(y, d - y) for y in range(8) if 0 <= d - y < 8]
        order += cells if d % 2 else cells[::-1]
    return [8 * y + x for y, x in order]


ZIGZAG = _zigzag()

DC_BITS = [[0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]]
DC_VALS = list(range(12))
AC_BITS = [[0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]]
AC_VALS = [bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8"
    "b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a4344"
    "45464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5"
    "b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")]
assert [len(v) for v in AC_VALS] == [162, 162] and [sum(b) for b in AC_BITS] == [162, 162] and [sum(b) for b in DC_BITS] == [12, 12]


def _codes(bits, vals):
    """Annex C: symbol -> (code, length)"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = [_codes(DC_BITS[c], DC_VALS) for c in range(2)]
AC_CODES = [_codes(AC_BITS[c], list(AC_VALS[c])) for c in range(2)]

# the DCT matrix of the contract: K[u][x] = round(4096 s(u) cos((2x + 1) u pi / 16))
_u, _x = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
KMAT = np.rint(4096.0 * np.where(_u == 0, np.sqrt(0.5), 1.0) * np.cos((2 * _x + 1) * _u * np.pi / 16)).astype(np.int64)
assert sorted(set(np.abs(KMAT).ravel().tolist())) == [799, 1567, 2276, 2896, 3406, 3784, 4017]


def quant_table(comp, quality):
    """libjpeg's quality rule on the Annex K table, natural order"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.array(K2 if comp else K1, np.int64) * scale + 50) // 100, 1, 255)


def header(h, w, quality):
    out = bytearray(b"\xff\xd8" + b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for c in range(2):
        out += b"\xff\xdb\x00\x43" + bytes([c]) + bytes(int(quant_table(c, quality)[k]) for k in ZIGZAG)
    out += b"\xff\xc0\x00\x11\x08" + bytes([h >> 8, h & 255, w >> 8, w & 255]) + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01"
    for c in range(2):
        out += b"\xff\xc4" + (19 + 12).to_bytes(2, "big") + bytes([c]) + bytes(DC_BITS[c]) + bytes(DC_VALS)
        out += b"\xff\xc4" + (19 + 162).to_bytes(2, "big") + bytes([0x10 | c]) + bytes(AC_BITS[c]) + AC_VALS[c]
    out += b"\xff\xdd\x00\x04\x00\x01"
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(out) == HEADER_BYTES
    return bytes(out)


def planes(frame):
    """padded, level-shifted Y [16 mh][16 mw] and Cb, Cr [8 mh][8 mw] (int64)"""
    h, w = frame.shape[:2]
    ph, pw = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    f = frame[np.minimum(np.arange(ph), h - 1)][:, np.minimum(np.arange(pw), w - 1)].astype(np.int64)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    assert min(y.min(), cb.min(), cr.min()) >= 0 and max(y.max(), cb.max(), cr.max()) <= 255

    def down(c):
        return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    return y - 128, down(cb) - 128, down(cr) - 128


def quantised_blocks(plane, comp, quality):
    """[rows / 8][cols / 8][64] quantised coefficients in zigzag order"""
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    p = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3)                  # [by][bx][y][x]
    r = (np.einsum("ux,abyx->abyu", KMAT, p) + (1 << 8)) >> 9             # rows: r[y][u]
    c = (np.einsum("vy,abyu->abvu", KMAT, r) + (1 << 13)) >> 14           # columns: c[v][u]
    assert np.abs(r).max() <= 8034 and np.abs(c).max() < (1 << 15) - 1020
    d = 8 * quant_table(comp, quality).reshape(8, 8)
    q = np.sign(c) * ((np.abs(c) + d // 2) // d)
    return q.reshape(hb, wb, 64)[:, :, ZIGZAG]


class _Bits(object):
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            v = (self.acc >> (self.n - 8)) & 255
            self.out.append(v)
            if v == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _value_bits(v, size):
    return (v if v >= 0 else v - 1) & ((1 << size) - 1)


def _code_block(q, comp, pred, bits, stats):
    diff = int(q[0]) - pred
    size = abs(diff).bit_length()
    bits.put(*DC_CODES[comp][size])
    if size:
        bits.put(_value_bits(diff, size), size)
    run = 0
    for v in q[1:].tolist():
        if v == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*AC_CODES[comp][0xF0])
            stats["zrl"] = stats.get("zrl", 0) + 1
            run -= 16
        size = abs(v).bit_length()
        stats["max_ac_category"] = max(stats.get("max_ac_category", 0), size)
        bits.put(*AC_CODES[comp][(run << 4) | size])
        bits.put(_value_bits(v, size), size)
        run = 0
    if run:
        bits.put(*AC_CODES[comp][0])
    return int(q[0])


def encode(frame_hw3, quality, stats=None):
    frame = np.asarray(frame_hw3)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3
    h, w = frame.shape[:2]
    assert 8 <= h <= 1024 and 8 <= w <= 1024 and 1 <= quality <= 100
    stats = {} if stats is None else stats
    y, cb, cr = planes(frame)
    qy, qcb, qcr = quantised_blocks(y, 0, quality), quantised_blocks(cb, 1, quality), quantised_blocks(cr, 1, quality)
    mh, mw = qcb.shape[:2]
    out = bytearray(header(h, w, quality))
    for m in range(mh * mw):
        my, mx = divmod(m, mw)
        bits, pred = _Bits(), 0
        for k in range(4):
            pred = _code_block(qy[2 * my + (k >> 1), 2 * mx + (k & 1)], 0, pred, bits, stats)
        _code_block(qcb[my, mx], 1, 0, bits, stats)
        _code_block(qcr[my, mx], 1, 0, bits, stats)
        bits.flush()
        stats["stuffed"] = stats.get("stuffed", 0) + bits.out.count(b"\xff\x00")
        out += bits.out
        out += b"\xff" + bytes([0xD9 if m == mh * mw - 1 else 0xD0 + (m & 7)])
    stats["mcus"] = stats.get("mcus", 0) + mh * mw
    return bytes(out)


# ---- the frames the CPU and the GPU tests share ---------------------------------------------------------------------------------
def frame(kind, h, w, seed=0):
    rs = np.random.RandomState(seed)
    if kind == "flat":
        return np.full((h, w, 3), (200, 30, 90), np.uint8)
    if kind == "noise":
        return rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    if kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    assert kind == "scene"
    # a synthetic scene: a floor gradient, a table-like rectangle, a disc and a thin line, with mild sensor noise
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([90 + 100 * yy / h, 120 + 60 * xx / w, 160 - 80 * yy / h], axis=2)
    img[(yy > 0.55 * h) & (xx > 0.2 * w) & (xx < 0.85 * w)] = (150, 110, 70)
    cy, cx, rad = (0.3 + 0.3 * rs.rand()) * h, (0.3 + 0.4 * rs.rand()) * w, 0.12 * min(h, w) + 1
    img[(yy - cy) ** 2 + (xx - cx) ** 2 < rad ** 2] = (220, 40, 40)
    img[np.abs(yy - 0.8 * xx * h / w - 2) < 0.8] = (20, 20, 20)
    return np.clip(img + rs.normal(0, 2.0, img.shape), 0, 255).astype(np.uint8)


KINDS = ("flat", "scene", "noise", "checker")
QUALITIES = (50, 75, 95, 100)
