"""A model of the energy VAD (include/cassnat_hip_vad.h) in Python integers and numpy, and of the five segmentation rules
of utils/vad.py - written from the definitions, not from the code under test.  ``mistake``: one of MISTAKES planted on purpose
(tests/test_vad_model.py shows that the case lists catch each)."""
import math

import numpy as np

FLOOR = 2.0 ** -23
MISTAKES = ("raw_ge", "window_unclipped", "drop_before_merge", "overlap_not_midpoint", "cut_last_minimum")


def num_frames(n, N, shift):
    return 0 if n < N else 1 + (n - N) // shift


def frame_num(x, N, remove_dc):
    """x: the N samples of one frame -> num as a Python integer."""
    xs = [int(v) for v in x]
    assert len(xs) == N
    S1, S2 = sum(xs), sum(v * v for v in xs)
    assert abs(S1) < 2 ** 27 and S2 <= 2 ** 41  # (the all -32768 frame of 2048 samples reaches 2^41)
    num = N * S2 - S1 * S1 if remove_dc else S2
    assert 0 <= num < 2 ** 52
    return num


def log_energy(num, N, remove_dc):
    E = float(num) / float(N) if remove_dc else float(num)
    return math.log(max(E, FLOOR))


def row_samples(off, samples, channels, staged_bytes):
    if off < 0 or off % 2 or samples <= 0 or off >= staged_bytes:
        return 0
    return min(samples, (staged_bytes - off) // (2 * channels))


def frame_energy(staged, off, samples, out_off, N, shift, channels, channel, remove_dc, max_frames, staged_bytes=None):
    """staged: uint8 array -> {index: (num, e)} of every frame that exists."""
    staged_bytes = len(staged) if staged_bytes is None else staged_bytes
    out = {}
    for o, s, at in zip(off, samples, out_off):
        n = row_samples(int(o), int(s), channels, staged_bytes)
        T = min(num_frames(n, N, shift), max_frames)
        if T == 0:
            continue
        x = np.frombuffer(staged[int(o):int(o) + 2 * n * channels].tobytes(), "<i2").reshape(n, channels)[:, channel]
        for t in range(T):
            m = frame_num(x[t * shift:t * shift + N], N, remove_dc)
            out[int(at) + t] = (m, log_energy(m, N, remove_dc))
    return out


def threshold(e, thr0, mean_scale):
    if mean_scale == 0 or len(e) == 0:
        return thr0
    return thr0 + mean_scale * (math.fsum(float(v) for v in e) / len(e))


def decide(e, thr0, mean_scale, context, proportion, mistake=None, thr=None):
    """-> (thr, [dec]) of one recording (``thr``: use this threshold instead of the model's own)."""
    T = len(e)
    thr = threshold(e, thr0, mean_scale) if thr is None else thr
    raw = [(v >= thr) if mistake == "raw_ge" else (v > thr) for v in e]
    dec = []
    for t in range(T):
        if mistake == "window_unclipped":
            num, den = sum(raw[k] for k in range(t - context, t + context + 1) if 0 <= k < T), 2 * context + 1
        else:
            win = range(max(0, t - context), min(T - 1, t + context) + 1)
            num, den = sum(raw[k] for k in win), len(win)
        dec.append(int(float(num) >= float(den) * proportion))
    return thr, dec


def margin(e, thr):
    """The distance of the nearest frame to the threshold."""
    return min(abs(float(v) - thr) for v in e) if len(e) else math.inf


def segment(dec, e, min_silence, min_speech, pad, max_segment, mistake=None):
    T = len(dec)
    runs, t = [], 0
    while t < T:
        if dec[t]:
            a = t
            while t < T and dec[t]:
                t += 1
            runs.append((a, t))
        else:
            t += 1

    def merge(rs):
        out = []
        for a, b in rs:
            if out and a - out[-1][1] < min_silence:
                out[-1] = (out[-1][0], b)
            else:
                out.append((a, b))
        return out

    def drop(rs):
        return [(a, b) for a, b in rs if b - a >= min_speech]

    runs = merge(drop(runs)) if mistake == "drop_before_merge" else drop(merge(runs))
    ends = [[max(0, a - pad), min(T, b + pad)] for a, b in runs]
    for i in range(len(runs) - 1):
        if ends[i][1] > ends[i + 1][0]:
            if mistake == "overlap_not_midpoint":
                ends[i][1] = ends[i + 1][0] = runs[i][1]
            else:
                ends[i][1] = ends[i + 1][0] = (runs[i][1] + runs[i + 1][0]) // 2
    out = []
    for a, b in ends:
        while b - a > max_segment:
            lo, hi = a + max_segment // 2, a + max_segment
            low = min(e[t] for t in range(lo, hi))
            where = [t for t in range(lo, hi) if e[t] == low]
            cut = where[-1] if mistake == "cut_last_minimum" else where[0]
            out.append((a, cut))
            a = cut
        out.append((a, b))
    return out


# ---- signals ---------------------------------------------------------------------------------------------------------------------------
def extreme_rows(N):
    """(name, N samples, num with DC removal, num without) worked out by hand: a constant frame (num = 0: the clamp), the all -32768
    frame (the largest S2; constant too) and alternating 32767 / -32768 (N even: S1 = -N / 2, S2 = N / 2 (32767^2 + 32768^2))."""
    rows = [("constant", np.full(N, 1234, np.int16), 0, N * 1234 * 1234),
            ("all_min", np.full(N, -32768, np.int16), 0, N * 32768 * 32768)]
    if N % 2 == 0:
        alt = np.tile(np.array([32767, -32768], np.int16), N // 2)
        S1, S2 = -(N // 2), (N // 2) * (32767 ** 2 + 32768 ** 2)
        rows.append(("alternating", alt, N * S2 - S1 * S1, S2))
    return rows


def recording(speech, rng_seed=7, gaps=(8000, 30000, 4000, 9000, 1200, 16000, 12000)):
    """The test recording: 0.5 s of +-3 noise, then 30000 / 9000 / 16000 samples of ``speech(n, seed)`` separated by 4000 and 1200
    samples of noise, then 12000 samples of noise (16 kHz)."""
    rng = np.random.RandomState(rng_seed)
    parts = []
    for k, n in enumerate(gaps):
        parts.append(rng.randint(-3, 4, n).astype(np.int16) if k % 2 == 0 else speech(n, 30 + k))
    return np.concatenate(parts)


# ---- case lists ------------------------------------------------------------------------------------------------------------------------
def crafted_e(T, seed=0):
    """T log-energies in quarters (0 .. 10); for T >= 4 the first four are 5.25, 5.25, 5.0, 5.0: with thr = 5.0 the raw decisions start
    1, 1, 0, 0 - e[2] == thr must say non-speech, and the window [0, 3] of t = 1 at context 2 is the exact tie 2 == 4 * 0.5."""
    e = np.random.RandomState(100 + T + seed).randint(0, 41, T) / 4.0
    if T >= 4:
        e[:4] = (5.25, 5.25, 5.0, 5.0)
    return e


def decide_cases():
    """(name, e, thr0, mean_scale, context, proportion) - thr is exact in every case: mean_scale 0, or a power-of-two T of quarters."""
    out = []
    for T in (1, 2, 65, 1000):
        for context in (0, 2, 64):
            for proportion in (0.0, 0.12, 0.5, 1.0):
                out.append(("T%d_c%d_p%g" % (T, context, proportion), crafted_e(T), 5.0, 0.0, context, proportion))
    for name, e in (("mean_T1", [6.0]), ("mean_T2", [4.0, 8.0]), ("mean_T2_tie", [6.0, 6.0]), ("mean_T64", crafted_e(64))):
        for context in (0, 2):
            out.append(("%s_c%d" % (name, context), np.array(e, np.float64), 3.0, 0.5, context, 0.5))
    return out


def segment_cases():
    """(name, dec, e, min_silence, min_speech, pad, max_segment, the segments worked out by hand)."""
    bits = lambda s: [int(c) for c in s]
    return [
        ("merge_then_drop", bits("10111000"), [0.0] * 8, 2, 2, 0, 100, [(0, 5)]),
        ("overlap_at_the_midpoint", bits("1111000011110000"), [0.0] * 16, 2, 2, 3, 100, [(0, 6), (6, 15)]),
        ("cut_at_the_first_minimum", [1] * 10, [5, 5, 5, 1, 1, 5, 5, 5, 5, 5], 1, 1, 0, 6, [(0, 3), (3, 6), (6, 10)]),
        ("pad_clipped", bits("0110"), [0.0] * 4, 1, 2, 5, 100, [(0, 4)]),
        ("short_dropped", bits("0100110"), [0.0] * 7, 1, 2, 0, 100, [(4, 6)]),
        ("nothing", bits("0000"), [0.0] * 4, 1, 1, 1, 100, []),
    ]


def frame_energy_fast(staged, off, samples, out_off, N, shift, channels, channel, remove_dc, max_frames, staged_bytes=None):
    """``frame_energy`` with the sums in numpy int64 (exact: every sum is below 2^63) - the same values, for the long rows."""
    staged_bytes = len(staged) if staged_bytes is None else staged_bytes
    out = {}
    for o, s, at in zip(off, samples, out_off):
        n = row_samples(int(o), int(s), channels, staged_bytes)
        T = min(num_frames(n, N, shift), max_frames)
        if T == 0:
            continue
        x = np.frombuffer(staged[int(o):int(o) + 2 * n * channels].tobytes(), "<i2").reshape(n, channels)[:, channel].astype(np.int64)
        win = np.lib.stride_tricks.sliding_window_view(x, N)[::shift][:T]
        S1, S2 = win.sum(1), (win * win).sum(1)
        for t in range(T):
            m = (N * int(S2[t]) - int(S1[t]) ** 2) if remove_dc else int(S2[t])
            out[int(at) + t] = (m, log_energy(m, N, remove_dc))
    return out


ENERGY_CONFIGS = [(400, 160, 1, 0), (200, 80, 1, 0), (1200, 480, 2, 1), (2048, 1, 1, 0), (1, 1, 1, 0), (400, 400, 8, 7)]
SENTINEL_NUM, SENTINEL_E, MARGIN = -77, -123.5, 5


def _samples_of(frames, N, shift):
    return (frames - 1) * shift + N


def energy_calls(cfg, seed=0):
    """The calls of one (N, shift, channels, channel): dicts with ``staged`` (uint8, noise in the gaps), ``staged_bytes``, ``off`` /
    ``samples`` / ``out_off`` (int32), ``max_frames`` and ``size``, the length of the outputs (MARGIN sentinels on both sides).
    Rows of N - 1, N, N + shift - 1 and N + shift samples, of 64, 65 and 1000 frames (the blocks of one row), the extreme rows, 1, 3
    and 33 rows in a call; the rows stand 0 / 2 / 6 / 14 bytes behind a multiple of 16, so that blocks start unaligned; the output
    order is a permutation of the rows; a last call cuts ``staged_bytes`` inside its last row, inside a sample frame."""
    N, shift, channels, channel = cfg
    rng = np.random.RandomState(1000 + N + 7 * shift + channels + seed)
    long_frames = 1000

    def noise(n):
        return rng.randint(-32768, 32768, n * channels).astype("<i2")

    def extreme(x):
        full = noise(len(x)).reshape(-1, channels)
        full[:, channel] = x
        return full.reshape(-1)

    pool = [noise(n) for n in (N - 1, N, N + shift - 1, N + shift) if n > 0]
    r64, r65 = noise(_samples_of(64, N, shift)), noise(_samples_of(65, N, shift))
    pool += [r64, r65]
    pool += [extreme(x) for _, x, _, _ in extreme_rows(N)]
    big = noise(_samples_of(long_frames, N, shift))
    calls = []
    for rows in ([r65], [pool[1], big, pool[2]], [pool[k % len(pool)] for k in range(33)]):
        calls.append(_lay_out(rows, channels, N, shift, rng))
    cut = _lay_out([r64, r65], channels, N, shift, rng)
    last = int(cut["off"][-1])
    cut["staged_bytes"] = last + 2 * channels * (_samples_of(40, N, shift) + 3) + 1  # (40 frames and three samples, then half a sample)
    calls.append(cut)
    return calls


def _lay_out(rows, channels, N, shift, rng):
    leads = (0, 2, 6, 14)
    off, at = [], 0
    for k, x in enumerate(rows):
        at = (at + 15) // 16 * 16 + leads[k % 4]
        off.append(at)
        at += x.nbytes
    staged = rng.randint(0, 256, (at + 15) // 16 * 16 + 16).astype(np.uint8)
    for o, x in zip(off, rows):
        staged[o:o + x.nbytes] = np.frombuffer(x.tobytes(), np.uint8)
    samples = [len(x) // channels for x in rows]
    frames = [num_frames(n, N, shift) for n in samples]
    order = rng.permutation(len(rows))
    out_off, fill = [0] * len(rows), MARGIN
    for r in order:
        out_off[r] = fill
        fill += frames[r]
    return {"staged": staged, "staged_bytes": at, "off": np.array(off, np.int32), "samples": np.array(samples, np.int32),
            "out_off": np.array(out_off, np.int32), "max_frames": max(1, max(frames)), "size": fill + MARGIN}


def e_bound(e):
    """|e - model| allowed: both logarithms are documented to 1 ulp and the argument is exact."""
    return 4 * 2.0 ** -52 * max(1.0, abs(e))


def thr_bound(e, mean_scale):
    T = len(e)
    return abs(mean_scale) * (T + 4) * 2.0 ** -52 * max(1.0, max((abs(float(v)) for v in e), default=0.0))
