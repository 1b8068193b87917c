"""The arithmetic contract of srlhip_jpeg_decode (include/srlhip.h) restated in numpy: decode(stream) -> uint8 [h][w][3].
A test helper like tests/jpeg_ref.py, whose tables and header it shares.  Written from the contract and from the published definitions
it names (ITU-T T.81 F.2.2 for the decoding procedure; the slow-integer inverse DCT, the triangle-filter upsampling and the fixed-point
colour conversion of the IJG library as their documentation states them) — nothing here is read from the product.  It decodes valid
streams only: anything else raises ValueError."""
import numpy as np

import jpeg_ref

_DC = [{(length, code): sym for sym, (code, length) in jpeg_ref.DC_CODES[c].items()} for c in range(2)]
_AC = [{(length, code): sym for sym, (code, length) in jpeg_ref.AC_CODES[c].items()} for c in range(2)]


def parse_header(data):
    """-> (h, w, [q_luma, q_chroma] in zigzag order); ValueError unless the 629 bytes are the encoder's layout"""
    if len(data) < jpeg_ref.HEADER_BYTES:
        raise ValueError("shorter than the header")
    h, w = int.from_bytes(data[163:165], "big"), int.from_bytes(data[165:167], "big")
    if not (8 <= h <= 1024 and 8 <= w <= 1024):
        raise ValueError("sides")
    want = bytearray(jpeg_ref.header(h, w, 50))
    got = bytearray(data[:jpeg_ref.HEADER_BYTES])
    tables = [np.array(got[25:89], np.int64), np.array(got[94:158], np.int64)]
    got[25:89] = want[25:89]
    got[94:158] = want[94:158]
    if got != want:
        raise ValueError("header layout")
    return h, w, tables


class _Bits(object):
    def __init__(self, payload):
        if b"\xff" in payload.replace(b"\xff\x00", b""):
            raise ValueError("marker inside an MCU")
        raw = payload.replace(b"\xff\x00", b"\xff")
        self.bits, self.at = "".join(format(b, "08b") for b in raw), 0

    def symbol(self, table):
        for length in range(1, 17):
            if self.at + length > len(self.bits):
                break
            sym = table.get((length, int(self.bits[self.at:self.at + length], 2)))
            if sym is not None:
                self.at += length
                return sym
        raise ValueError("no code")

    def value(self, size):
        if self.at + size > len(self.bits):
            raise ValueError("bits past the MCU's end")
        v = int(self.bits[self.at:self.at + size], 2)
        self.at += size
        return v if v >= 1 << (size - 1) else v - (1 << size) + 1


def _block(bits, comp, pred, q):
    """-> (dequantised coefficients [64] in natural order, the block's DC before dequantisation)"""
    out = np.zeros(64, np.int64)
    size = bits.symbol(_DC[comp])
    dc = pred + (bits.value(size) if size else 0)
    out[0] = dc * q[0]
    k = 1
    while k < 64:
        rs = bits.symbol(_AC[comp])
        run, size = rs >> 4, rs & 15
        if size == 0:
            if run != 15:
                break
            k += 16
            if k > 63:
                raise ValueError("ZRL past the block")
            continue
        k += run
        if k > 63:
            raise ValueError("coefficient index past 63")
        out[jpeg_ref.ZIGZAG[k]] = bits.value(size) * q[k]
        k += 1
    return out, dc


def coefficients(data, h, w, tables):
    """-> dequantised coefficients [mh][mw][6][8][8]"""
    mh, mw = (h + 15) // 16, (w + 15) // 16
    body, out = data[jpeg_ref.HEADER_BYTES:], np.zeros((mh * mw, 6, 64), np.int64)
    for m in range(mh * mw):
        trailer = b"\xff" + bytes([0xD9 if m == mh * mw - 1 else 0xD0 + (m & 7)])
        # the first 0xFF that is not followed by 0x00 ends the MCU
        at = 0
        while True:
            at = body.index(b"\xff", at)
            if body[at + 1:at + 2] != b"\x00":
                break
            at += 2
        if body[at:at + 2] != trailer:
            raise ValueError("marker {} of {}".format(m, mh * mw))
        bits, body, pred = _Bits(body[:at]), body[at + 2:], 0
        for k in range(4):
            out[m, k], pred = _block(bits, 0, pred, tables[0])
        out[m, 4], _ = _block(bits, 1, 0, tables[1])
        out[m, 5], _ = _block(bits, 1, 0, tables[1])
    if body:
        raise ValueError("bytes behind EOI")
    assert np.abs(out).max() < 1 << 15
    return out.reshape(mh, mw, 6, 8, 8)


def _idct_1d(x, shift):
    """the slow-integer 8-point inverse DCT along the LAST axis: constants round(c * 2^13)"""
    i0, i1, i2, i3, i4, i5, i6, i7 = (x[..., k] for k in range(8))
    z1 = (i2 + i6) * 4433
    t2, t3 = z1 - i6 * 15137, z1 + i2 * 6270
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z1, z2, z3, z4 = i7 + i1, i5 + i3, i7 + i3, i5 + i1
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = i7 * 2446, i5 * 16819, i3 * 25172, i1 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    out = np.stack([t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3], axis=-1)
    assert np.abs(out).max() < (1 << 31) - (1 << 17)           # the contract's 32-bit sums do not wrap on valid streams
    return (out + (1 << (shift - 1))) >> shift


def samples(coef):
    """[...][8][8] coefficients -> [...][8][8] samples"""
    cols = np.swapaxes(_idct_1d(np.swapaxes(coef, -1, -2), 11), -1, -2)       # columns first, 2 extra bits kept
    v = _idct_1d(cols, 18)
    assert v.min() >= -512 and v.max() <= 511
    return np.clip(v + 128, 0, 255)


def _upsample(c):
    """fancy 2x2 upsampling of the real chroma samples [ch][cw] -> [2 ch][2 cw]"""
    ch, cw = c.shape
    rows = np.arange(2 * ch)
    near, far = rows >> 1, np.clip(np.where(rows & 1, (rows >> 1) + 1, (rows >> 1) - 1), 0, ch - 1)
    s = 3 * c[near] + c[far]                                    # [2 ch][cw]
    left, right = np.concatenate([s[:, :1], s[:, :-1]], axis=1), np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((2 * ch, 2 * cw), np.int64)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    return out


def decode(data):
    data = bytes(data)
    h, w, tables = parse_header(data)
    s = samples(coefficients(data, h, w, tables))               # [mh][mw][6][8][8]
    mh, mw = s.shape[:2]
    y = s[:, :, :4].reshape(mh, mw, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(16 * mh, 16 * mw)
    cb = s[:, :, 4].transpose(0, 2, 1, 3).reshape(8 * mh, 8 * mw)
    cr = s[:, :, 5].transpose(0, 2, 1, 3).reshape(8 * mh, 8 * mw)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    y, cb, cr = y[:h, :w], _upsample(cb[:ch, :cw])[:h, :w] - 128, _upsample(cr[:ch, :cw])[:h, :w] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


# ---- the frames and streams the CPU and the GPU tests share -----------------------------------------------------------------------
KINDS = ("gradient", "noise", "black", "white", "checker", "quadrants")
QUALITIES = (10, 50, 95)


def frame(kind, h, w, seed=0):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "gradient":                                      # smooth: long zero runs, ZRL, EOB
        return np.stack([255 * yy // (h - 1), 255 * xx // (w - 1), 255 - 255 * (yy + xx) // (h + w - 2)], axis=2).astype(np.uint8)
    if kind == "noise":                                         # all 63 AC terms
        return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    if kind == "black":
        return np.zeros((h, w, 3), np.uint8)
    if kind == "white":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "checker":                                       # the largest categories and the clamps
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    assert kind == "quadrants"                                  # one saturated colour per quadrant: chroma edges
    colours = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0]], np.uint8)
    return colours[2 * (yy >= h // 2) + (xx >= w // 2)]
