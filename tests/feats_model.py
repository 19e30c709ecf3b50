"""The matrix compression of DESIGN.md 7n in numpy / Python integers: the model the host twin (cn_compress_feats_host), the kernel
(cn_op_compress_feats) and the tool (bin/make_fbank) are held to, byte for byte.  numpy rounds every float32 operation on its own,
which is what the definition asks for.  ``mistake`` plants one of five deliberate errors (tests/test_feats_model.py shows that the
case list catches each)."""
import math
import struct

import numpy as np

f32 = np.float32
U16_INC = f32(1.52590218966964e-05)
MISTAKES = ("3T/4", "0.5", "<=", "no_forcing", "product64")
OK, NO_ROWS, NOT_FINITE, BAD_SPAN = 0, 1, 2, 3


def payload_bytes(T, F):
    if T < 0 or F < 1:
        return 0
    return 16 + 8 * F + T * F if T > 8 else 16 + 2 * T * F


def layout(lens, F, tmax):
    """Byte offsets (multiples of 16) of the payloads laid one behind the other, and the end of the last."""
    offs, o = [], 0
    for n in lens:
        o = (o + 15) // 16 * 16
        offs.append(o)
        o += payload_bytes(max(0, min(int(n), tmax)), F)
    return np.asarray(offs, np.int32), o


def trunc_clamp(d, hi):
    """clamp(int(d), 0, hi) with a truncating conversion; a NaN gives 0."""
    d = np.asarray(d, np.float64)
    with np.errstate(invalid="ignore"):
        low, high = ~(d >= 1.0), d >= hi
        return np.where(low, 0, np.where(high, hi, np.trunc(np.where(low | high, 0.0, d)))).astype(np.int64)


def _product(a, k, mistake):
    if mistake == "product64":
        return a.astype(np.float64) * float(k)
    return (a * f32(k)).astype(np.float64)


def u16(v, mn, rng, mistake=None):
    with np.errstate(all="ignore"):
        f = (np.asarray(v, f32) - mn) / rng
        f = np.where(f < 0, f32(0), np.where(f > 1, f32(1), f)).astype(f32)
        return trunc_clamp(_product(f, 65535, mistake) + (0.5 if mistake == "0.5" else 0.499), 65535)


def global_range(x):
    """(min, range) of the global header, or None where the range is not finite."""
    with np.errstate(all="ignore"):
        mn, mx = f32(x.min()) + f32(0), f32(x.max())
        if mx == mn:
            mx = mn + (f32(1) + abs(mn))
        rng = f32(mx - mn)
    return (mn, rng) if np.isfinite(rng) else None


def column_headers(codes, T, mistake=None):
    """codes (T, F) int -> (F, 4) header codes."""
    s = np.sort(codes, axis=0)
    q = T // 4
    c = s[[0, q, 3 * T // 4 if mistake == "3T/4" else 3 * q, T - 1]].T.astype(np.int64)
    if mistake == "no_forcing":
        return c
    h = np.empty_like(c)
    h[:, 0] = np.minimum(c[:, 0], 65532)
    h[:, 1] = np.minimum(np.maximum(c[:, 1], h[:, 0] + 1), 65533)
    h[:, 2] = np.minimum(np.maximum(c[:, 2], h[:, 1] + 1), 65534)
    h[:, 3] = np.maximum(c[:, 3], h[:, 2] + 1)
    return h


def quartiles(h, mn, rng):
    """P0..P100 (F, 4) float32 as the reader dequantises the header codes."""
    return (mn + (rng * U16_INC) * h.astype(f32)).astype(f32)


def _segment(v, lo, hi, codes, top, mistake):
    with np.errstate(all="ignore"):
        return trunc_clamp(_product(((v - lo) / (hi - lo)).astype(f32), codes, mistake) + 0.5, top)


def column_bytes(x, p, mistake=None):
    """x (T, F) float32, p (F, 4) -> (T, F) byte values."""
    p0, p25, p75, p100 = (p[:, k][None, :] for k in range(4))
    lo = _segment(x, p0, p25, 64, 64, mistake)
    mid = 64 + _segment(x, p25, p75, 128, 128, mistake)
    hi = 192 + _segment(x, p75, p100, 63, 63, mistake)
    first = (x <= p25) if mistake == "<=" else (x < p25)
    return np.where(first, lo, np.where(x < p75, mid, hi))


def compress(x, mistake=None):
    """A float32 (T, F) matrix -> (status, token, payload bytes); token and payload are None unless the status is 0."""
    x = np.ascontiguousarray(x, f32)
    T, F = x.shape
    if T < 1:
        return NO_ROWS, None, None
    g = global_range(x) if np.isfinite(x).all() else None
    if g is None:
        return NOT_FINITE, None, None
    mn, rng = g
    head = struct.pack("<ffii", mn, rng, T, F)
    codes = u16(x, mn, rng, mistake)
    if T <= 8:
        return OK, b"CM2 ", head + codes.astype("<u2").tobytes()
    h = column_headers(codes, T, mistake)
    b = column_bytes(x, quartiles(h, mn, rng), mistake)
    return OK, b"CM ", head + h.astype("<u2").tobytes() + np.ascontiguousarray(b.T).astype(np.uint8).tobytes()


def compress_batch(feats, lens, out_off, out, mistake=None):
    """The entry points' contract on a padded (rows, Tmax, F) batch: payload r into ``out`` (uint8, in place) at out_off[r], -> the
    int32 status words.  Rows at or behind an utterance's length are not looked at."""
    rows, tmax, F = feats.shape
    status = np.zeros(rows, np.int32)
    for r in range(rows):
        T = min(int(lens[r]), tmax)
        if T < 1:
            status[r] = NO_ROWS
            continue
        o = int(out_off[r])
        if o < 0 or o % 16 or o + payload_bytes(T, F) > out.size:
            status[r] = BAD_SPAN
            continue
        status[r], _, payload = compress(feats[r, :T], mistake)
        if status[r] == OK:
            out[o:o + len(payload)] = np.frombuffer(payload, np.uint8)
    return status


def steps(x, payload):
    """Per value of a compressed (T, F) matrix the code width of the segment it was coded in (at bytes 64 and 192 the wider of the two
    neighbouring segments), and the range: the terms of the round-trip cap."""
    T, F = x.shape
    mn, rng = (f32(v) for v in struct.unpack("<ff", payload[:8]))
    if T <= 8:
        return np.full((T, F), float(rng) / 65535), float(rng)
    h = np.frombuffer(payload[16:16 + 8 * F], "<u2").reshape(F, 4)
    p = quartiles(h, mn, rng).astype(np.float64)
    w = np.stack([(p[:, 1] - p[:, 0]) / 64, (p[:, 2] - p[:, 1]) / 128, (p[:, 3] - p[:, 2]) / 63])  # (3, F)
    b = np.frombuffer(payload[16 + 8 * F:], np.uint8).reshape(F, T).T
    cols = np.broadcast_to(np.arange(F), (T, F))
    seg = np.where(b <= 64, 0, np.where(b <= 192, 1, 2))
    step = w[seg, cols]
    step = np.where(b == 64, np.maximum(w[0, cols], w[1, cols]), step)
    step = np.where(b == 192, np.maximum(w[1, cols], w[2, cols]), step)
    return step, float(rng)


def stats(stored):
    """(2, F) float64: the sum and the sum of squares of the columns of what an archive holds, in the order the kernel and its host
    twin add them: sixteen partial sums (row t into partial t % 16, rows in order), then the partials from the first to the last."""
    v = np.asarray(stored, np.float64)
    out = np.zeros((2, v.shape[1]))
    for k in range(16):
        if v[k::16].shape[0]:
            out += np.stack([np.cumsum(v[k::16], axis=0)[-1], np.cumsum(v[k::16] * v[k::16], axis=0)[-1]])
    return out


def exact_stats(stored):
    v = np.asarray(stored, np.float64)
    return np.array([[math.fsum(v[:, c]) for c in range(v.shape[1])], [math.fsum(v[:, c] * v[:, c]) for c in range(v.shape[1])]])


def stats_bound(stored):
    """(T - 1) * 2^-53 * (sum|x|, sum x^2): what any order of float64 additions stays within (the squares of float32 values are exact)."""
    v = np.asarray(stored, np.float64)
    cols = range(v.shape[1])
    return (v.shape[0] - 1) * 2.0 ** -53 * np.array([[math.fsum(np.abs(v[:, c])) for c in cols], [math.fsum(v[:, c] * v[:, c]) for c in cols]])
