"""The contract of srlhip_jpeg_decode_baseline (include/srlhip.h) restated in numpy and plain Python: decode(stream) -> uint8 [h][w][3]
and statistics of what the stream's entropy-coded data held.  A test helper like tests/jpeg_decode_ref.py, whose inverse DCT,
upsampling and frame kinds it shares, and tests/jpeg_ref.py, whose Annex K.3 tables it shares.  Written from the contract and from
ITU-T T.81 (B.2 for the segments, F.2.2 for the decoding procedure, E.2.4 / F.2.2.4 for restarts) — nothing here is read from the
product.  It decodes accepted, valid streams only: anything else raises ValueError, whose text starts with "header" for what the
contract gives status 1 and with "data" for status 3."""
import numpy as np

import jpeg_decode_ref
import jpeg_ref

# (class, kind) -> {(length, code): symbol}; kind 0 luminance, 1 chrominance
_CODES = {(0, c): {(length, code): sym for sym, (code, length) in jpeg_ref.DC_CODES[c].items()} for c in range(2)}
_CODES.update({(1, c): {(length, code): sym for sym, (code, length) in jpeg_ref.AC_CODES[c].items()} for c in range(2)})
# what a DHT segment holds for each of them: 16 BITS, then HUFFVAL
_K3 = {(0, c): bytes(jpeg_ref.DC_BITS[c]) + bytes(jpeg_ref.DC_VALS) for c in range(2)}
_K3.update({(1, c): bytes(jpeg_ref.AC_BITS[c]) + bytes(jpeg_ref.AC_VALS[c]) for c in range(2)})


def parse(data):
    """-> dict(h, w, sampling 420 / 444, ri, data_start, q [3] tables in zigzag order, dc [3] and ac [3] code tables of the components)"""
    data = bytes(data)
    if not data:
        raise ValueError("empty")
    if data[:2] != b"\xff\xd8":
        raise ValueError("header: no SOI")
    pos, dqt, dht, sof, ri = 2, {}, {}, None, 0
    for _ in range(64):
        if pos + 4 > len(data) or data[pos] != 0xFF:
            raise ValueError("header: no marker segment at {}".format(pos))
        m, length = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        if length < 2 or pos + 2 + length > len(data):
            raise ValueError("header: segment length")
        body = data[pos + 4:pos + 2 + length]
        if 0xE0 <= m <= 0xED or m in (0xEF, 0xFE):
            pass
        elif m == 0xDB:
            while body:
                if len(body) < 65 or body[0] > 3:
                    raise ValueError("header: DQT")
                dqt[body[0]] = np.array(list(body[1:65]), np.int64)
                body = body[65:]
        elif m == 0xC0:
            if sof is not None or len(body) != 15 or body[0] != 8 or body[5] != 3:
                raise ValueError("header: SOF0")
            h, w = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            comps = [tuple(body[6 + 3 * c:9 + 3 * c]) for c in range(3)]
            if not (8 <= h <= 1024 and 8 <= w <= 1024) or [c[0] for c in comps] != [1, 2, 3] or any(c[2] > 3 for c in comps):
                raise ValueError("header: SOF0 sides or components")
            if [c[1] for c in comps] not in ([0x22, 0x11, 0x11], [0x11, 0x11, 0x11]):
                raise ValueError("header: sampling")
            sof = (h, w, 420 if comps[0][1] == 0x22 else 444, [c[2] for c in comps])
        elif m == 0xC4:
            while body:
                if len(body) < 17 or body[0] >> 4 > 1 or body[0] & 15 > 1:
                    raise ValueError("header: DHT")
                n, tc = 17 + sum(body[1:17]), body[0] >> 4
                kinds = [k for k in range(2) if body[1:n] == _K3[(tc, k)]]
                if len(body) < n or not kinds:
                    raise ValueError("header: a Huffman table that is not Annex K.3's")
                dht[(tc, body[0] & 15)] = kinds[0]
                body = body[n:]
        elif m == 0xDD:
            if len(body) != 2:
                raise ValueError("header: DRI")
            ri = int.from_bytes(body, "big")
        elif m == 0xDA:
            if sof is None or len(body) != 10 or body[0] != 3 or tuple(body[7:10]) != (0, 63, 0):
                raise ValueError("header: SOS")
            dc, ac, q = [], [], []
            for c in range(3):
                td, ta = body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15
                if body[1 + 2 * c] != c + 1 or (0, td) not in dht or (1, ta) not in dht or sof[3][c] not in dqt:
                    raise ValueError("header: SOS selectors")
                dc.append(_CODES[(0, dht[(0, td)])])
                ac.append(_CODES[(1, dht[(1, ta)])])
                q.append(dqt[sof[3][c]])
            return dict(h=sof[0], w=sof[1], sampling=sof[2], ri=ri, data_start=pos + 2 + length, q=q, dc=dc, ac=ac)
        else:
            raise ValueError("header: marker {:#x}".format(m))
        pos += 2 + length
    raise ValueError("header: more than 64 segments")


class _Interval(object):
    """the bits from `pos` up to the first 0xFF that is not followed by 0x00 (or up to the stream's end), stuffing removed"""

    def __init__(self, data, pos, stats):
        at = pos
        while True:
            at = data.find(b"\xff", at)
            if at < 0 or data[at + 1:at + 2] != b"\x00":
                break
            at += 2
            stats["stuffed"] = stats.get("stuffed", 0) + 1
        self.marker_at = len(data) if at < 0 else at
        raw = data[pos:self.marker_at].replace(b"\xff\x00", b"\xff")
        self.bits, self.at = "".join(format(b, "08b") for b in raw), 0

    def symbol(self, table):
        for length in range(1, 17):
            if self.at + length > len(self.bits):
                raise ValueError("data: bits past the data's end")
            sym = table.get((length, int(self.bits[self.at:self.at + length], 2)))
            if sym is not None:
                self.at += length
                return sym
        raise ValueError("data: no code")

    def value(self, size):
        if self.at + size > len(self.bits):
            raise ValueError("data: bits past the data's end")
        v = int(self.bits[self.at:self.at + size], 2)
        self.at += size
        return v if v >= 1 << (size - 1) else v - (1 << size) + 1


def _wrap16(v):
    return (int(v) + (1 << 15)) % (1 << 16) - (1 << 15)


def _block(bits, dc, ac, pred, q, stats):
    """-> (dequantised coefficients [64] in natural order, the block's DC before dequantisation)"""
    out = np.zeros(64, np.int64)
    size = bits.symbol(dc)
    if size > 11:
        raise ValueError("data: DC category")
    stats["max_dc_category"] = max(stats.get("max_dc_category", 0), size)
    pred += bits.value(size) if size else 0
    out[0] = _wrap16(pred * q[0])
    k = 1
    while k < 64:
        rs = bits.symbol(ac)
        run, size = rs >> 4, rs & 15
        if size == 0:
            if run != 15:
                break
            stats["zrl"] = stats.get("zrl", 0) + 1
            k += 16
            if k > 63:
                raise ValueError("data: ZRL past the block")
            continue
        k += run
        if k > 63:
            raise ValueError("data: coefficient index past 63")
        stats["max_ac_category"] = max(stats.get("max_ac_category", 0), size)
        out[jpeg_ref.ZIGZAG[k]] = _wrap16(bits.value(size) * q[k])
        k += 1
    return out, pred


def coefficients(data, hd, stats):
    """-> dequantised coefficients [n_mcus][blocks per MCU][64]"""
    big = hd["sampling"] == 420
    side, comps = (16, [0, 0, 0, 0, 1, 2]) if big else (8, [0, 1, 2])
    nm = -(-hd["h"] // side) * -(-hd["w"] // side)
    out = np.zeros((nm, len(comps), 64), np.int64)
    bits, pred, restarts = _Interval(data, hd["data_start"], stats), [0, 0, 0], 0
    for m in range(nm):
        if m and hd["ri"] and m % hd["ri"] == 0:
            # the rest of the current byte is dropped; nothing but the marker may follow
            if len(bits.bits) - bits.at >= 8:
                raise ValueError("data: data bytes where restart {} must stand".format(restarts))
            if data[bits.marker_at:bits.marker_at + 2] != bytes([0xFF, 0xD0 + restarts % 8]):
                raise ValueError("data: restart marker {}".format(restarts))
            bits, pred, restarts = _Interval(data, bits.marker_at + 2, stats), [0, 0, 0], restarts + 1
        elif m and any(pred):
            stats["max_carried_dc_{}".format(hd["sampling"])] = max(stats.get("max_carried_dc_{}".format(hd["sampling"]), 0), max(abs(p) for p in pred))
        for b, c in enumerate(comps):
            out[m, b], pred[c] = _block(bits, hd["dc"][c], hd["ac"][c], pred[c], hd["q"][c], stats)
    stats["restarts"] = max(stats.get("restarts", 0), restarts)
    return out


def decode(data, stats=None):
    """-> uint8 [h][w][3].  stats (a dict, updated over calls): zrl, stuffed (FF 00 pairs met), max_dc_category, max_ac_category, restarts
    (the most restart markers one stream held), max_carried_dc_420 / _444 (the largest |DC predictor| carried across an MCU border)"""
    data = bytes(data)
    stats = {} if stats is None else stats
    hd = parse(data)
    h, w = hd["h"], hd["w"]
    s = jpeg_decode_ref.samples(coefficients(data, hd, stats).reshape(-1, 8, 8))
    if hd["sampling"] == 420:
        mh, mw = -(-h // 16), -(-w // 16)
        s = s.reshape(mh, mw, 6, 8, 8)
        y = s[:, :, :4].reshape(mh, mw, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(16 * mh, 16 * mw)
        cb = s[:, :, 4].transpose(0, 2, 1, 3).reshape(8 * mh, 8 * mw)
        cr = s[:, :, 5].transpose(0, 2, 1, 3).reshape(8 * mh, 8 * mw)
        ch, cw = (h + 1) // 2, (w + 1) // 2
        cb, cr = jpeg_decode_ref._upsample(cb[:ch, :cw]), jpeg_decode_ref._upsample(cr[:ch, :cw])
    else:
        mh, mw = -(-h // 8), -(-w // 8)
        y, cb, cr = (s.reshape(mh, mw, 3, 8, 8)[:, :, c].transpose(0, 2, 1, 3).reshape(8 * mh, 8 * mw) for c in range(3))
    y, cb, cr = y[:h, :w], cb[:h, :w] - 128, cr[:h, :w] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


# ---- the fixture both test files share -------------------------------------------------------------------------------------------
def load_fixture(path):
    """tests/golden/jpeg_baseline_pillow.npz -> list of dict(name, h, w, kind, quality, subsampling, restart, stream bytes, frame)"""
    z = np.load(path)
    cases = []
    for i, name in enumerate(z["names"].tolist()):
        h, w, kind, quality, subsampling, restart = name.split(",")
        frame = z["frame_{}".format(i)]
        frame.setflags(write=False)
        cases.append(dict(name=name, h=int(h), w=int(w), kind=kind, quality=int(quality), subsampling=int(subsampling), restart=restart,
                          stream=z["stream_{}".format(i)].tobytes(), frame=frame))
    return cases


def load_refused(path):
    """-> {what: stream bytes} of the fixture's streams that must be refused at the header: progressive, optimised, greyscale, 422"""
    z = np.load(path)
    return {k[len("refused_"):]: z[k].tobytes() for k in z.files if k.startswith("refused_")}


def pick(cases, **want):
    """the first fixture case with these fields"""
    return next(c for c in cases if all(c[k] == v for k, v in want.items()))


def with_app14(data):
    """the stream with an Adobe APP14 segment (transform 0) spliced in behind SOI"""
    return data[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + data[2:]


def damaged(data, positions=16):
    """single-byte damage, 0x00 and 0xFF, at `positions` places spread over header and data -> list of (position, value, bytes)"""
    out = []
    for pos in np.linspace(2, len(data) - 3, positions).round().astype(int).tolist():
        for value in (0x00, 0xFF):
            d = bytearray(data)
            d[pos] = value
            out.append((pos, value, bytes(d)))
    return out
