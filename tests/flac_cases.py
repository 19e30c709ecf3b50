"""The FLAC streams the tests of the FLAC input path share (a helper, not a test): a handful of utterances written by the model
(tests/flac_model.py) from explicit recipes that between them hold every construct the decoder implements - see ``utterances``."""
import functools

import numpy as np

import flac_model as fm


def walk(n, channels=1, seed=0, step=40, limit=30000):
    """A random walk on the int16 scale, (n, channels)."""
    rng = np.random.default_rng(seed)
    return np.clip(np.cumsum(rng.integers(-step, step + 1, (n, channels)), axis=0), -limit, limit).astype(np.int64)


def fixed(order, po=0, **kw):
    return dict(type="fixed", order=order, partition_order=po, **kw)


def lpc(coefs, precision, shift, po=0, **kw):
    return dict(type="lpc", order=len(coefs), coefs=list(coefs), precision=precision, shift=shift, partition_order=po, **kw)


def frame(pcm, subs, assignment=None, **kw):
    pcm = np.asarray(pcm, np.int64).reshape(len(pcm), -1)
    return dict(pcm=pcm, assignment=pcm.shape[1] - 1 if assignment is None else assignment, subframes=subs, **kw)


def unary_run_residuals():
    """Fixed order 0 with Rice parameter 0 codes the residual r as u zeros and a one (u = 2r, or -2r - 1): runs of 31, 32, 33, 63,
    64, 65 and 100 zeros, the group (395 bits, 3 mod 8) eight times over - every run starts at each of the 8 bit phases, and crosses
    the 32- and 64-bit boundaries of a word-wise reader at each."""
    runs = [31, 32, 33, 63, 64, 65, 100]
    assert sum(q + 1 for q in runs) % 8 == 3
    return [q // 2 if q % 2 == 0 else -(q + 1) // 2 for _ in range(8) for q in runs]


def block_sizes():
    """Mono, variable block size: 16 and 17 with the explicit 8- and 16-bit codes, 4097 (16-bit), 192, 576, 4096, 4608, a last frame of
    ONE sample; fixed orders 0-4 in turn."""
    sizes = [(16, 6), (16, 7), (17, 6), (17, 7), (4097, 7), (192, None), (576, None), (4096, None), (4608, None), (1, None)]
    x = walk(sum(n for n, _ in sizes), 1, seed=1)
    out, at = [], 0
    for k, (n, code) in enumerate(sizes):
        out.append(frame(x[at:at + n], [fixed(min(k % 5, n))], bs_code=code))
        at += n
    return out, True


def subframe_types():
    """Mono, fixed block size 192, last frame 15 samples: constant, verbatim, fixed 0-4, LPC of orders 1, 2, 8, 12, 32 with precisions
    1, 12, 15 and shifts 0, 14; partition orders 0, 1, 4 (the largest 192 allows with order <= 12 is 4: 16 partitions of 12)."""
    rng = np.random.default_rng(2)
    x = walk(192 * 13 + 15, 1, seed=2)
    subs = [dict(type="constant"), dict(type="verbatim")] + [fixed(o, po) for o, po in zip(range(5), (0, 1, 4, 0, 1))]
    subs += [lpc([-1], 1, 0), lpc([2, -1], 12, 0, po=1), lpc(rng.integers(-2000, 2000, 8), 15, 14, po=4),
             lpc(rng.integers(-1300, 1300, 12), 12, 14, po=4), lpc(rng.integers(-500, 500, 32), 15, 14, po=1), lpc([0], 1, 14)]
    out = []
    for k, sub in enumerate(subs):
        chunk = x[192 * k:192 * (k + 1)].copy()
        if sub["type"] == "constant":
            chunk[:] = -12345
        out.append(frame(chunk, [sub]))
    out.append(frame(x[192 * 13:], [fixed(3)]))
    assert len(subs) == 13
    return out, False


def rice_and_escapes():
    """Mono, variable block size: Rice parameters 0 and 14 (4-bit method), 15 and 30 (5-bit method); the unary runs; escapes of
    widths 0, 1 and 16; the largest partition order a block allows (4096 samples, order 12: one residual per partition) with the first
    partition EMPTY (fixed order 1); a block of 16 in 4 partitions with order 4 (first partition empty again); wasted bits 1 and 15."""
    rng = np.random.default_rng(3)
    quiet = rng.integers(-3, 4, (64, 1))
    loud = walk(64, 1, seed=4, step=3000)
    runs = np.array(unary_run_residuals(), np.int64)[:, None]
    esc = np.concatenate([np.zeros(16), rng.integers(-1, 1, 16), rng.integers(-32768, 32768, 32)]).astype(np.int64)[:, None]
    out = [frame(quiet, [fixed(0, 1, params=[0, 0])]), frame(loud, [fixed(0, 1, params=[14, 14])]),
           frame(loud, [fixed(1, 1, method=1, params=[15, 30])]), frame(quiet, [fixed(2, 0, method=1, params=[30])]),
           frame(runs, [fixed(0, 0, params=[0])]), frame(esc, [fixed(0, 2, escapes={0: 0, 1: 1, 2: 16, 3: 16})]),
           frame(esc, [fixed(0, 2, method=1, escapes={0: 0, 2: 16}, params=[0, 3, 0, 14])]),
           frame(walk(4096, 1, seed=5), [fixed(1, 12)]), frame(walk(16, 1, seed=6), [fixed(4, 2)]),
           frame(walk(64, 1, seed=7, limit=16000) * 2, [fixed(2, 0, wasted=1)]),
           frame(rng.integers(-1, 1, (64, 1)) * 32768, [dict(type="verbatim", wasted=15)]),
           frame(rng.integers(-1, 1, (64, 1)) * 32768, [fixed(1, 0, wasted=15)])]
    return out, True


def stereo():
    """Two channels, fixed block size 64, last frame 15: independent, left/side, side/right and mid/side - with L = 32767 / R = -32768
    (the side needs 17 bits) and odd L + R under mid/side -, a side channel escaped at width 17, and the order-32, 15-bit-precision
    LPC on a 17-bit side channel whose sum leaves 32 bits (32 x 16383 x 65535 is about 2^35)."""
    x = walk(64 * 9 + 15, 2, seed=8, step=900)
    x[64:128, 0], x[64:128, 1] = 32767, -32768  # left/side at the extreme
    x[128:192:2, 0] += 1                        # odd sums under mid/side
    extreme = np.empty((64, 2), np.int64)
    extreme[:, 0], extreme[:, 1] = 32767, -32768
    extreme[40:, 0] = 32000
    out = [frame(x[0:64], [fixed(2), fixed(1)], 1), frame(x[64:128], [fixed(0), fixed(1)], 8), frame(x[128:192], [fixed(2), fixed(2, 1)], 10),
           frame(x[192:256], [fixed(1), fixed(2)], 9), frame(x[256:320], [fixed(2), fixed(0, 0, escapes={0: 17})], 8),
           frame(extreme, [fixed(0), lpc([16383] * 32, 15, 14, method=1)], 8), frame(extreme, [lpc([-16384] * 32, 15, 14, method=1), fixed(0)], 9),
           frame(extreme, [fixed(1), dict(type="verbatim")], 10), frame(x[512:576], [dict(type="verbatim"), fixed(4, 2)], 10),
           frame(x[576:], [fixed(2), fixed(3)], 10)]
    return out, False


def many_channels(channels, seed):
    """3 or 8 independent channels, fixed block size 48, last frame 5."""
    x = walk(48 * 3 + 5, channels, seed=seed)
    return [frame(x[at:at + 48], [fixed((c + at) % 5 if at + 48 <= len(x) else 1) for c in range(channels)]) for at in range(0, len(x), 48)], False


@functools.lru_cache(maxsize=None)
def utterances():
    """-> list of dicts: ``name``, ``data`` (the file's bytes), ``first`` (offset of the first frame), ``offsets`` (of every frame, from
    there), ``pcm`` ('<i2' (samples, channels)), ``channels``, ``rate``, ``variable``."""
    out = []
    for name, (frames, variable) in (("sizes", block_sizes()), ("types", subframe_types()), ("rice", rice_and_escapes()), ("stereo", stereo()),
                                     ("three", many_channels(3, 9)), ("eight", many_channels(8, 10))):
        data, first, offsets, pcm = fm.write_stream(frames, rate=16000, variable=variable)
        out.append(dict(name=name, data=data, first=first, offsets=offsets, pcm=pcm, channels=pcm.shape[1], rate=16000, variable=variable,
                        sizes=[f["pcm"].shape[0] for f in frames]))
    return out
