"""Float64 restatement of Kaldi's LinearResample as ResampleWaveform configures it (kaldi-asr/kaldi src/feat/resample.cc:
num_zeros = 6, cutoff = 0.99 * 0.5 * min(rates)), the definition csrc/resample.hip is held to.  Plain Python and numpy; no GPU, no
library.  The reference tree never opens a sound file, so - as for the fbank front-end - parity is pinned to the published
algorithm."""
import math

import numpy as np

NUM_ZEROS = 6
PAIRS = [(8000, 16000), (48000, 16000), (44100, 16000), (22050, 16000), (11025, 16000), (16000, 8000)]


def units(fi, fo):
    g = math.gcd(fi, fo)
    return fi // g, fo // g


def cutoff_of(fi, fo):
    return 0.99 * 0.5 * min(fi, fo)


def filt_win(d, fi, fo):
    """filt(d) * win(d): the windowed sinc at time offset d (seconds)."""
    cutoff = cutoff_of(fi, fo)
    window_width = NUM_ZEROS / (2.0 * cutoff)
    win = 0.5 * (1.0 + math.cos(2.0 * math.pi * cutoff / NUM_ZEROS * d)) if abs(d) < window_width else 0.0
    filt = math.sin(2.0 * math.pi * cutoff * d) / (math.pi * d) if d != 0.0 else 2.0 * cutoff
    return filt * win


def table(fi, fo):
    """-> (in_unit, out_unit, first [out_unit], weights: list of float64 arrays, one per phase)."""
    in_unit, out_unit = units(fi, fo)
    if fi == fo:
        return 1, 1, [0], [np.array([1.0])]
    window_width = NUM_ZEROS / (2.0 * cutoff_of(fi, fo))
    first, weights = [], []
    for i in range(out_unit):
        t = i / fo
        lo, hi = math.ceil((t - window_width) * fi), math.floor((t + window_width) * fi)
        first.append(lo)
        weights.append(np.array([filt_win(j / fi - t, fi, fo) / fi for j in range(lo, hi + 1)], np.float64))
    return in_unit, out_unit, first, weights


def num_samples(fi, fo, n):
    """GetNumOutputSamples with flush = true."""
    tick = fi // math.gcd(fi, fo) * fo
    L = n * (tick // fi)
    if L <= 0:
        return 0
    tpo = tick // fo
    last = L // tpo
    if last * tpo == L:
        last -= 1
    return last + 1


def resample(x, fi, fo, weights32=False):
    """x: one channel -> (y float64 [num_samples], bound_sum float64: sum_j |w_j x_j| per output).  ``weights32``: the weights
    rounded to float32 first (what the device multiplies with)."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    in_unit, out_unit, first, weights = table(fi, fo)
    if weights32:
        weights = [w.astype(np.float32).astype(np.float64) for w in weights]
    count = num_samples(fi, fo, n)
    y, s = np.zeros(count), np.zeros(count)
    if count == 0:
        return y, s
    lo, hi = min(first), max(f + len(w) for f, w in zip(first, weights))
    pad_l = max(0, -lo)
    u_max = (count - 1) // out_unit
    xp = np.zeros(pad_l + max(n, u_max * in_unit + hi) + 1)
    xp[pad_l:pad_l + n] = x
    for p in range(out_unit):
        ks = np.arange(p, count, out_unit)
        if ks.size == 0:
            continue
        base = pad_l + first[p] + (ks // out_unit) * in_unit
        for j, w in enumerate(weights[p]):  # ascending j
            term = w * xp[base + j]
            y[ks] += term
            s[ks] += np.abs(term)
    return y, s


def direct(x, fi, fo, k):
    """Output k as the sum over ALL input samples j of x[j] * filt(j / fi - k / fo) * win(.) / fi (win is 0 outside the window)."""
    return sum(float(x[j]) * filt_win(j / fi - k / fo, fi, fo) / fi for j in range(len(x)))


def pick(data, channels, c):
    """Channel c of an interleaved data chunk."""
    return np.asarray(data)[c::channels]
