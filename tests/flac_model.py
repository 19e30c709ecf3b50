"""A bit-exact FLAC (RFC 9639) writer and reader in Python / numpy, written for the tests of the FLAC input path (a model, not a test).

The WRITER takes an explicit recipe per frame and channel, so that a test can force every construct of the format instead of hoping
that an encoder picks it: subframe type, order, coefficients, precision and shift, wasted bits, partition order, Rice method and
parameters, escapes, the channel assignment, the block size and how it is coded, fixed or variable blocking.  ``write_stream`` puts
`fLaC`, STREAMINFO (with the MD5 of the interleaved little-endian PCM) and optional PADDING / VORBIS_COMMENT / SEEKTABLE / other
blocks in front of the frames, and also returns where every frame starts.

The READER (``read_stream``) decodes with Python integers and verifies every CRC-8, every CRC-16 and the MD5.

``encode_fast`` is a vectorised fixed-predictor + Rice writer of mono streams for the timing tool, which needs thousands of
utterances; everything else here is plain Python loops over tens of frames.

A frame recipe is a dict: ``pcm`` int array (block size, channels); ``assignment`` 0-7 (independent; must be channels - 1) or 8 / 9 /
10; ``subframes`` one dict per coded channel; ``bs_code`` None (the shortest code that fits) or 6 / 7 to force the explicit 8- / 16-bit
form; ``rate_code`` None (0: from STREAMINFO) or a code 1-14; ``size_code`` None (4) or 0.  A subframe recipe: ``type`` "constant" /
"verbatim" / "fixed" / "lpc"; ``order``; ``coefs``, ``precision``, ``shift`` (lpc); ``wasted``; ``partition_order``; ``method`` 0 / 1;
``params`` one Rice parameter per partition (None: the cheapest); ``escapes`` {partition: width} of raw partitions.
"""
import hashlib
import struct

import numpy as np

FIXED = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
CODE_RATES = {v: k for k, v in RATE_CODES.items()}
SIZE_CODES = {0: 0, 1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}


def _crc_table(poly, bits):
    top, mask = 1 << (bits - 1), (1 << bits) - 1
    out = []
    for i in range(256):
        c = i << (bits - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        out.append(c)
    return out


_CRC8, _CRC16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def crc8(data):
    c = 0
    for b in data:
        c = _CRC8[c ^ b]
    return c


def crc16(data):
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _CRC16[(c >> 8) ^ b]
    return c


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def write(self, v, k):
        if k:
            self.acc = (self.acc << k) | (int(v) & ((1 << k) - 1))
            self.n += k

    def unary(self, q):
        self.write(1, q + 1)

    def bytes(self):
        pad = -self.n % 8
        return ((self.acc << pad).to_bytes((self.n + pad) // 8, "big")) if self.n else b""


def coded_number(v):
    """The UTF-8-style code of the frame / sample number (up to 36 bits, 1-7 bytes)."""
    if v < 0x80:
        return bytes([v])
    for nbytes in range(2, 8):
        if v < 1 << (5 * nbytes + 1):
            out = [(0xFF << (8 - nbytes)) & 0xFF | (v >> (6 * (nbytes - 1)))]
            out += [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(nbytes - 2, -1, -1)]
            return bytes(out)
    raise ValueError("coded number %d" % v)


def _bs_code(bs, force=None):
    if force in (6, 7):
        return force
    if bs == 192:
        return 1
    for n in range(2, 6):
        if bs == 576 << (n - 2):
            return n
    for n in range(8, 16):
        if bs == 256 << (n - 8):
            return n
    return 6 if bs <= 256 else 7


def frame_header(number, bs, assignment, variable=False, bs_code=None, rate_code=None, size_code=None, rate=None):
    code = _bs_code(bs, bs_code)
    rc = 0 if rate_code is None else rate_code
    out = bytes([0xFF, 0xF8 | int(variable), (code << 4) | rc, (assignment << 4) | ((4 if size_code is None else size_code) << 1)]) + coded_number(number)
    if code == 6:
        out += bytes([bs - 1])
    elif code == 7:
        out += struct.pack(">H", bs - 1)
    if rc == 12:
        out += bytes([rate // 1000])
    elif rc == 13:
        out += struct.pack(">H", rate)
    elif rc == 14:
        out += struct.pack(">H", rate // 10)
    return out + bytes([crc8(out)])


def residual_of(x, sub):
    """The residual (Python ints, from sample ``order`` on) of the channel signal ``x`` under the recipe's predictor."""
    kind, order = sub["type"], int(sub.get("order", 0))
    if kind == "fixed":
        coefs, shift = FIXED[order], 0
    else:
        coefs, shift = [int(c) for c in sub["coefs"]], int(sub["shift"])
        assert len(coefs) == order
    return [x[i] - (sum(c * x[i - 1 - j] for j, c in enumerate(coefs)) >> shift) for i in range(order, len(x))]


def _rice_bits(res, k):
    return sum(((r << 1) if r >= 0 else ((-r) << 1) - 1) >> k for r in res) + len(res) * (1 + k)


def write_residual(bw, res, bs, order, sub):
    method, po = int(sub.get("method", 0)), int(sub.get("partition_order", 0))
    pbits = 4 + method
    esc = (1 << pbits) - 1
    assert bs % (1 << po) == 0 and (bs >> po) >= order
    params, escapes = sub.get("params"), sub.get("escapes", {})
    bw.write(method, 2)
    bw.write(po, 4)
    at = 0
    for part in range(1 << po):
        cnt = (bs >> po) - (order if part == 0 else 0)
        chunk = res[at:at + cnt]
        at += cnt
        if part in escapes:
            width = int(escapes[part])
            assert all(-(1 << (width - 1)) <= r < (1 << (width - 1)) for r in chunk) if width else all(r == 0 for r in chunk)
            bw.write(esc, pbits)
            bw.write(width, 5)
            for r in chunk:
                bw.write(r, width)
            continue
        k = int(params[part]) if params is not None else min(range(esc), key=lambda kk: _rice_bits(chunk, kk))
        assert 0 <= k < esc
        bw.write(k, pbits)
        for r in chunk:
            u = (r << 1) if r >= 0 else ((-r) << 1) - 1
            bw.unary(u >> k)
            bw.write(u, k)
    assert at == len(res)


def write_subframe(bw, x, bps, sub):
    x = [int(v) for v in x]
    kind, wasted, bs = sub["type"], int(sub.get("wasted", 0)), len(x)
    code = {"constant": 0, "verbatim": 1}.get(kind)
    order = int(sub.get("order", 0))
    if kind == "fixed":
        code = 8 | order
    elif kind == "lpc":
        code = 32 | (order - 1)
    bw.write(0, 1)
    bw.write(code, 6)
    bw.write(1 if wasted else 0, 1)
    if wasted:
        assert all(v % (1 << wasted) == 0 for v in x)
        bw.unary(wasted - 1)
        x = [v >> wasted for v in x]
        bps -= wasted
    assert all(-(1 << (bps - 1)) <= v < (1 << (bps - 1)) for v in x), "the samples do not fit %d bits" % bps
    if kind == "constant":
        assert all(v == x[0] for v in x)
        bw.write(x[0], bps)
    elif kind == "verbatim":
        for v in x:
            bw.write(v, bps)
    else:
        for v in x[:order]:
            bw.write(v, bps)
        if kind == "lpc":
            prec = int(sub["precision"])
            assert 1 <= prec <= 15 and all(-(1 << (prec - 1)) <= int(c) < (1 << (prec - 1)) for c in sub["coefs"])
            bw.write(prec - 1, 4)
            bw.write(int(sub["shift"]), 5)
            for c in sub["coefs"]:
                bw.write(int(c), prec)
        write_residual(bw, residual_of(x, sub), bs, order, sub)


def channel_signals(pcm, assignment):
    """The signals the subframes code, with their sample sizes, for 16-bit ``pcm`` (block size, channels)."""
    pcm = np.asarray(pcm, np.int64)
    if assignment < 8:
        assert pcm.shape[1] == assignment + 1
        return [(pcm[:, c], 16) for c in range(pcm.shape[1])]
    left, right = pcm[:, 0], pcm[:, 1]
    side = left - right
    if assignment == 8:
        return [(left, 16), (side, 17)]
    if assignment == 9:
        return [(side, 17), (right, 16)]
    return [((left + right) >> 1, 16), (side, 17)]


def write_frame(recipe, number, variable=False, rate=None):
    pcm = np.asarray(recipe["pcm"], np.int64)
    if pcm.ndim == 1:
        pcm = pcm[:, None]
    assignment = int(recipe.get("assignment", pcm.shape[1] - 1))
    head = frame_header(number, pcm.shape[0], assignment, variable, recipe.get("bs_code"), recipe.get("rate_code"), recipe.get("size_code"), rate)
    bw = BitWriter()
    for (x, bps), sub in zip(channel_signals(pcm, assignment), recipe["subframes"]):
        write_subframe(bw, x, bps, sub)
    body = head + bw.bytes()
    return body + struct.pack(">H", crc16(body))


def metadata_block(kind, body, last=False):
    return bytes([(0x80 if last else 0) | kind]) + len(body).to_bytes(3, "big") + body


def streaminfo(rate, channels, bits, total, min_bs, max_bs, min_frame=0, max_frame=0, md5=b"\0" * 16):
    packed = (rate << 44) | ((channels - 1) << 41) | ((bits - 1) << 36) | total
    return struct.pack(">HH", min_bs, max_bs) + min_frame.to_bytes(3, "big") + max_frame.to_bytes(3, "big") + packed.to_bytes(8, "big") + md5


def write_stream(frames, rate=16000, variable=False, blocks=(), total=None, bits=16, streaminfo_channels=None, streaminfo_rate=None):
    """-> (the file's bytes, offset of the first frame, [offset of every frame from there], the interleaved int16 PCM (samples,
    channels)).  ``blocks``: (kind, body) metadata blocks behind STREAMINFO (1 PADDING, 3 SEEKTABLE, 4 VORBIS_COMMENT, ...);
    ``total``: the STREAMINFO total (None: the true one; 0: unknown)."""
    chunks, offsets, at, first = [], [], 0, 0
    for k, rec in enumerate(frames):
        bs = np.asarray(rec["pcm"]).shape[0]
        data = write_frame(rec, first if variable else k, variable, rate)
        offsets.append(at)
        chunks.append(data)
        at += len(data)
        first += bs
    pcm = np.concatenate([np.asarray(r["pcm"], np.int64).reshape(np.asarray(r["pcm"]).shape[0], -1) for r in frames]).astype("<i2")
    sizes = [np.asarray(r["pcm"]).shape[0] for r in frames]
    info = streaminfo(rate if streaminfo_rate is None else streaminfo_rate, pcm.shape[1] if streaminfo_channels is None else streaminfo_channels,
                      bits, pcm.shape[0] if total is None else total, min(sizes), max(sizes), min(map(len, chunks)), max(map(len, chunks)),
                      hashlib.md5(pcm.tobytes()).digest())
    head = b"fLaC" + metadata_block(0, info, last=not blocks)
    for i, (kind, body) in enumerate(blocks):
        head += metadata_block(kind, body, last=i == len(blocks) - 1)
    return head + b"".join(chunks), len(head), offsets, pcm


# ---- the reader ---------------------------------------------------------------------------------------------------------------
class BitReader:
    def __init__(self, data, pos=0):
        self.data, self.pos, self.acc, self.n = data, pos, 0, 0

    def read(self, k):
        while self.n < k:
            self.acc = (self.acc << 8) | self.data[self.pos]
            self.pos += 1
            self.n += 8
        self.n -= k
        v = self.acc >> self.n
        self.acc &= (1 << self.n) - 1
        return v

    def signed(self, k):
        v = self.read(k)
        return v - (1 << k) if k and v >> (k - 1) else v

    def unary(self):
        q = 0
        while not self.read(1):
            q += 1
        return q

    def align(self):
        assert self.read(self.n % 8) == 0, "non-zero padding bits"
        assert self.n == 0 or self.n % 8 == 0
        self.pos -= self.n // 8
        self.acc = self.n = 0
        return self.pos


def read_metadata(data):
    """-> (dict of STREAMINFO's fields, offset of the first frame, [(kind, body)])."""
    assert data[:4] == b"fLaC"
    pos, blocks, last = 4, [], False
    while not last:
        last, kind = bool(data[pos] & 0x80), data[pos] & 0x7F
        size = int.from_bytes(data[pos + 1:pos + 4], "big")
        blocks.append((kind, data[pos + 4:pos + 4 + size]))
        pos += 4 + size
    assert blocks[0][0] == 0
    body = blocks[0][1]
    packed = int.from_bytes(body[10:18], "big")
    info = {"min_bs": struct.unpack(">H", body[:2])[0], "max_bs": struct.unpack(">H", body[2:4])[0], "rate": packed >> 44,
            "channels": ((packed >> 41) & 7) + 1, "bits": ((packed >> 36) & 31) + 1, "total": packed & ((1 << 36) - 1), "md5": body[18:34]}
    return info, pos, blocks


def read_frame(data, pos, info):
    """One frame at ``pos`` -> (pcm (block size, channels) int64, next position, header dict); CRC-8 and CRC-16 are verified."""
    start = pos
    assert data[pos] == 0xFF and data[pos + 1] & 0xFE == 0xF8
    variable = data[pos + 1] & 1
    bs_code, rate_code = data[pos + 2] >> 4, data[pos + 2] & 15
    assignment, size_code = data[pos + 3] >> 4, (data[pos + 3] >> 1) & 7
    assert not data[pos + 3] & 1 and bs_code != 0 and rate_code != 15 and assignment <= 10
    pos += 4
    b0 = data[pos]
    ones = 0
    while b0 & (0x80 >> ones):
        ones += 1
    assert ones != 1 and ones <= 7
    number = b0 & (0x7F >> ones)
    pos += 1
    for _ in range(max(0, ones - 1)):
        assert data[pos] & 0xC0 == 0x80
        number = (number << 6) | (data[pos] & 0x3F)
        pos += 1
    if bs_code == 1:
        bs = 192
    elif bs_code <= 5:
        bs = 576 << (bs_code - 2)
    elif bs_code == 6:
        bs, pos = data[pos] + 1, pos + 1
    elif bs_code == 7:
        bs, pos = struct.unpack(">H", data[pos:pos + 2])[0] + 1, pos + 2
    else:
        bs = 256 << (bs_code - 8)
    rate = info["rate"] if rate_code == 0 else CODE_RATES.get(rate_code)
    if rate_code == 12:
        rate, pos = data[pos] * 1000, pos + 1
    elif rate_code in (13, 14):
        rate, pos = struct.unpack(">H", data[pos:pos + 2])[0] * (1 if rate_code == 13 else 10), pos + 2
    assert crc8(data[start:pos]) == data[pos], "frame header CRC-8"
    pos += 1
    bits = SIZE_CODES[size_code] or info["bits"]
    channels = assignment + 1 if assignment < 8 else 2
    br = BitReader(data, pos)
    sig = []
    for c in range(channels):
        bps = bits + (1 if (assignment, c) in ((8, 1), (9, 0), (10, 1)) else 0)
        assert br.read(1) == 0
        code = br.read(6)
        wasted = br.unary() + 1 if br.read(1) else 0
        bps -= wasted
        if code == 0:
            x = [br.signed(bps)] * bs
        elif code == 1:
            x = [br.signed(bps) for _ in range(bs)]
        else:
            if code & 32:
                order = (code & 31) + 1
            else:
                assert code & 0x38 == 8 and (code & 7) <= 4
                order = code & 7
            x = [br.signed(bps) for _ in range(order)]
            if code & 32:
                prec = br.read(4) + 1
                assert prec != 16
                shift = br.signed(5)
                assert shift >= 0
                coefs = [br.signed(prec) for _ in range(order)]
            else:
                coefs, shift = FIXED[order], 0
            method = br.read(2)
            assert method < 2
            pbits, po = 4 + method, br.read(4)
            assert bs % (1 << po) == 0
            res = []
            for part in range(1 << po):
                cnt = (bs >> po) - (order if part == 0 else 0)
                assert cnt >= 0
                k = br.read(pbits)
                if k == (1 << pbits) - 1:
                    width = br.read(5)
                    res += [br.signed(width) for _ in range(cnt)]
                else:
                    for _ in range(cnt):
                        u = (br.unary() << k) | br.read(k)
                        res.append((u >> 1) ^ -(u & 1))
            for r in res:
                i = len(x)
                x.append(r + (sum(cf * x[i - 1 - j] for j, cf in enumerate(coefs)) >> shift))
        sig.append([v << wasted for v in x])
    end = br.align()
    assert crc16(data[start:end]) == struct.unpack(">H", data[end:end + 2])[0], "frame CRC-16"
    a = np.array(sig, dtype=object).T
    if assignment == 8:
        a[:, 1] = a[:, 0] - a[:, 1]
    elif assignment == 9:
        a[:, 0] = a[:, 0] + a[:, 1]
    elif assignment == 10:
        m = (a[:, 0] * 2) | (a[:, 1] & 1)
        a[:, 0], a[:, 1] = (m + a[:, 1]) >> 1, (m - a[:, 1]) >> 1
    return a.astype(np.int64), end + 2, {"variable": variable, "number": number, "bs": bs, "rate": rate, "assignment": assignment, "bits": bits}


def read_stream(data):
    """-> (pcm (samples, channels) '<i2', STREAMINFO dict, [frame offsets from the first frame]); verifies CRCs, numbering and MD5."""
    info, first, _ = read_metadata(data)
    pos, parts, offsets, samples = first, [], [], 0
    while pos < len(data):
        offsets.append(pos - first)
        pcm, pos, h = read_frame(data, pos, info)
        assert h["number"] == (samples if h["variable"] else len(parts)) and h["rate"] == info["rate"] and h["bits"] == info["bits"]
        assert pcm.shape[1] == info["channels"]
        parts.append(pcm)
        samples += pcm.shape[0]
    out = np.concatenate(parts)
    assert out.min() >= -32768 and out.max() <= 32767
    out = out.astype("<i2")
    assert info["total"] in (0, samples)
    assert hashlib.md5(out.tobytes()).digest() == info["md5"], "MD5 of the PCM"
    return out, info, offsets


# ---- convenience recipes ------------------------------------------------------------------------------------------------------
def fixed_sub(order=2, partition_order=0, **kw):
    return dict(type="fixed", order=order, partition_order=partition_order, **kw)


def simple_frames(pcm, bs, order=2, assignment=None, partition_order=0):
    """``pcm`` (samples, channels) cut into frames of ``bs`` (the last one shorter), every channel a fixed predictor."""
    pcm = np.asarray(pcm, np.int64).reshape(len(pcm), -1)
    out = []
    for at in range(0, pcm.shape[0], bs):
        chunk = pcm[at:at + bs]
        n = chunk.shape[0]
        o = min(order, n)
        po = partition_order if n % (1 << partition_order) == 0 and (n >> partition_order) >= o else 0
        out.append({"pcm": chunk, "assignment": pcm.shape[1] - 1 if assignment is None else assignment,
                    "subframes": [fixed_sub(o, po) for _ in range(pcm.shape[1])]})
    return out


# ---- the vectorised writer of the timing tool ---------------------------------------------------------------------------------
def _bits_of(values, width):
    """(n,) non-negative ints -> (n, width) bits, most significant first."""
    return ((np.asarray(values, np.int64)[:, None] >> np.arange(width - 1, -1, -1)) & 1).astype(np.uint8)


def encode_fast(pcm, rate=16000, bs=4096, order=2, crc16_fn=crc16):
    """Mono int16 ``pcm`` -> (file bytes, offset of the first frame): fixed predictor of ``order``, one Rice partition with the
    parameter chosen from the mean magnitude, every step numpy.  ``crc16_fn``: a faster CRC-16 (polynomial 0x8005) when there is one."""
    pcm = np.asarray(pcm, np.int64)
    chunks = []
    for k, at in enumerate(range(0, len(pcm), bs)):
        x = pcm[at:at + bs]
        o = min(order, len(x))
        res = x.copy()
        for _ in range(o):
            res = np.diff(res)
        u = np.where(res >= 0, res << 1, ((-res) << 1) - 1)
        mean = float(u.mean()) if len(u) else 0.0
        kk = min(14, max(0, int(np.log2(mean + 1))))
        q = u >> kk
        head = np.concatenate([_bits_of([0], 1)[0], _bits_of([8 | o], 6)[0], [0]] + [_bits_of(x[:o] & 0xFFFF, 16).ravel()] +
                              [_bits_of([0], 2)[0], _bits_of([0], 4)[0], _bits_of([kk], 4)[0]]).astype(np.uint8)
        width = q + 1 + kk
        ends = np.cumsum(width)
        bits = np.zeros(int(ends[-1]) if len(ends) else 0, np.uint8)
        if len(u):
            starts = ends - width
            bits[starts + q] = 1
            for j in range(kk):
                bits[starts + q + 1 + j] = (u >> (kk - 1 - j)) & 1
        body = frame_header(k, len(x), 0) + np.packbits(np.concatenate([head, bits])).tobytes()
        chunks.append(body + struct.pack(">H", crc16_fn(body)))
    raw = pcm.astype("<i2")
    sizes = [min(bs, len(pcm) - at) for at in range(0, len(pcm), bs)]
    info = streaminfo(rate, 1, 16, len(pcm), bs, bs, min(map(len, chunks)), max(map(len, chunks)), hashlib.md5(raw.tobytes()).digest())
    del sizes
    head = b"fLaC" + metadata_block(0, info, last=True)
    return head + b"".join(chunks), len(head)
