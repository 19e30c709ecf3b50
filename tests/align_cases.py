"""The inputs tests/test_align_model.py (models against the oracle, no GPU) and tests/test_gpu_align_kernels.py (kernels against the
models) share: the smallest shapes that reach each branch of the alignment and hypothesis kernels, rows crafted per case."""
import numpy as np

from align_model import collapse_shift, subsampled

ALIGN_TP = [1, 2, 12, 255, 256, 257, 513]  # the 256-wide scan: one chunk short by one, exactly one, one frame of a second, a third
TRIGGERS = [(0, 0), (1, 0), (0, 1), (1, 1)]
ALIGN_FORMS = ["raw_path", "src_mod", "utt_meta", "no_trigger", "no_trigger+utt_meta", "src_mod+utt_meta", "raw_path+utt_meta"]
ALIGN_ROWS = ["full length", "holes in the mask", "no token", "token on the last valid frame", "tokens on frames 254 / 255 / 256",
              "src_size 0", "src_size one short of the mask", "masked frame with a non-blank label", "ragged"]


def align_case(Tp, B=9):
    """best (B, Tp), mask (B, Tp) bool, ratio (B,) float32, lens (B,): row r as ALIGN_ROWS[r % 9] names it."""
    rng = np.random.default_rng(1000 + Tp)
    t = np.arange(Tp)
    best = rng.integers(1, 6, size=(B, Tp)) * (rng.random((B, Tp)) < 0.5)
    lens = rng.integers(1, Tp + 1, size=B)
    for b in range(B):
        if b % 9 in (0, 1, 4, 5):  # (5: fully valid, so that the frame its EOS row wraps to shows)
            lens[b] = Tp
        if b % 9 == 7:
            lens[b] = max(1, Tp - 2)
    mask = t[None, :] < lens[:, None]
    ratio = (lens / Tp).astype(np.float32)
    for b in range(B):
        kind = b % 9
        if kind == 1 and Tp >= 3:
            mask[b, rng.choice(np.arange(1, Tp), size=min(3, Tp - 2), replace=False)] = False
        if kind == 2:
            best[b] = 0
        if kind == 3:  # a token that starts on the very last valid frame: the shift drops it past the mask
            best[b, lens[b] - 1] = 5
            if lens[b] >= 2:
                best[b, lens[b] - 2] = 0
        if kind == 4:  # tokens whose shifted frames are the last of a scan chunk and the first of the next
            best[b] = 0
            for k, f in enumerate((254, 255, 256) if Tp > 254 else (Tp // 2,)):
                if f < Tp:
                    best[b, f] = 1 + k
        if kind == 5:
            ratio[b] = np.float32(0.4 / Tp)
        if kind == 6:
            ratio[b] = np.float32((lens[b] - 0.6) / Tp)
        if kind == 7:  # zeroed in the plain form, kept under raw_path
            hole = lens[b] // 2
            mask[b, hole] = lens[b] < 2
            best[b, hole] = 5
            if hole >= 1:
                best[b, hole - 1] = 2
            best[b, lens[b]:] = 4
    return best.astype(np.int64), mask, ratio, lens


def meta_of(rows, tps):
    """(sum rows, 4) records (frames, T', first, one past the last) of batches of `rows` utterances with `tps` subsampled frames."""
    out, lo = [], 0
    for r, tp in zip(rows, tps):
        out += [[4 * tp - 3, tp, lo, lo + r]] * r
        lo += r
    meta = np.array(out, np.int64)
    assert all(subsampled(int(f)) == tp for f, tp in meta[:, :2])
    return meta


def align_form_case(Tp, form):
    """The keyword arguments of align_model (and of the kernel's descriptor) for one of ALIGN_FORMS at width Tp."""
    rng = np.random.default_rng(2000 + Tp + 7 * ALIGN_FORMS.index(form))
    G = 3
    Bs = 4 if "src_mod" in form else 9
    best, mask, ratio, lens = align_case(Tp, Bs)
    kw = dict(left=int(rng.integers(0, 2)), right=int(rng.integers(0, 2)))
    if "src_mod" in form:  # G paths per utterance: path 0 the case's own, the others random
        more = rng.integers(1, 6, size=((G - 1) * Bs, Tp)) * (rng.random(((G - 1) * Bs, Tp)) < 0.4)
        best = np.concatenate([best, more])
        kw["src_mod"] = Bs
    if "raw_path" in form:  # per-frame labels of a forced alignment: runs of a label, blanks between, not zeroed on masked frames
        best = np.repeat(rng.integers(0, 6, size=(Bs, Tp // 2 + 1)), 2, axis=1)[:, :Tp]
        best[2] = 0
        best[7, lens[7] // 2] = 5
        kw["raw_path"] = True
    tps = np.full(Bs, Tp)
    if "utt_meta" in form:  # three batches of T' {Tp, Tp - 3, 1}: an utterance's frames at or past its batch's T' do not exist
        meta = meta_of([2, 1, 1] if Bs == 4 else [4, 3, 2], [Tp, Tp - 3, 1])
        tps = meta[:, 1]
        for b in range(Bs):  # (the ratios are those of the batch's own width: src_size = (ratio * T').long())
            tp = int(meta[b, 1])
            mask[b, tp:] = False
            n = min(int(lens[b]), tp)
            ratio[b] = np.float32({5: 0.4, 6: n - 0.6}.get(b % 9, n) / tp)
        mask[Bs - 1, 0] = False  # (an utterance without a valid frame)
        for b in range(best.shape[0]):  # what lies behind a batch's own width is never read: poison it
            best[b, int(meta[b % Bs, 1]):] = 3
        u, tp = (5, Tp - 3) if Bs == 9 else (2, Tp - 3)  # a token that starts on the LAST frame of its own batch: the shift drops it
        mask[u, :tp] = True
        best[u::Bs, tp - 1], best[u::Bs, tp - 2] = 4, 0
        kw["utt_meta"] = meta
    if "raw_path" in form:  # the given label counts: the path's own, or one more (labels that did not fit: the EOS row is then
        # the forced frame alone - the only rows in which the frame a src_size of 0 wraps to shows, row 5 among them)
        kw["ylen_in"] = np.array([(collapse_shift(best[b:b + 1, :tps[b]]) != 0).sum() for b in range(Bs)]) + (np.arange(Bs) % 2)
    if "no_trigger" in form:
        kw["no_trigger"] = True
    return dict(best=best, mask=mask, ratio=ratio, **kw)


# ---------------------------------------------------------------------------------------------------------- forced alignment
VITERBI_SHAPES = [(6, 40, 12, 9), (3, 300, 12, 130), (4, 1, 5, 1)]  # (B, Tp, V, ymax): 2 ymax + 1 = 261 > 256 in the second


def viterbi_case(B, Tp, V, ymax):
    """logp (B, Tp, V) float32, mask, ratio, labels (B, ld) int with ld = ymax + 2 and garbage behind each row's count (the kernel
    must read them as blank), ys (B, ymax) zero padded (the reference's input), ylens."""
    rng = np.random.default_rng(3000 + Tp)
    x = rng.standard_normal((B, Tp, V)).astype(np.float32) * 2
    logp = (x - np.log(np.exp(x.astype(np.float64)).sum(-1, keepdims=True))).astype(np.float32)
    mask = np.ones((B, Tp), bool)
    ratio = np.ones(B, np.float32)
    ys = np.zeros((B, ymax), np.int64)
    if Tp == 40:
        ylens = np.array([0, 7, 8, 4, 3, 2])          # ymax 9 is larger than every count
        ys[1, :7] = 3                                  # all labels equal: 13 frames at least
        ys[2, :8] = rng.integers(1, V, size=8)
        ratio[2] = np.float32(5.5 / Tp)                # 8 labels, 5 frames: the trace walks through unreachable states
        ys[3, :4] = [2, 2, 5, 2]
        mask[3, [6, 7, 19, 30]] = False                # masked frames in the middle
        ratio[3] = np.float32(36.5 / Tp)
        ys[4, :3] = [4, 1, 1]
        ratio[4] = np.float32(0.4 / Tp)                # xb = 0
        ys[5, :2] = [7, 9]
        ratio[5] = np.float32(1.5 / Tp)                # xb = 1; rows 0 and 1: xb = Tp
    elif Tp == 300:
        ylens = np.array([130, 100, 130])
        ys[0] = rng.integers(1, V, size=130)           # (12 labels: many neighbours repeat)
        ys[1, :100] = rng.integers(1, V, size=100)
        mask[1, rng.choice(np.arange(1, Tp), size=25, replace=False)] = False
        ys[2] = rng.integers(1, 3, size=130)
        ratio[2] = np.float32(200.5 / Tp)              # 130 labels of two kinds do not fit 200 frames
    else:
        ylens = np.array([0, 1, 1, 1])
        ys[1:, 0] = [3, 2, 4]
        ratio[2] = np.float32(0.4)                     # xb = 0 on a single frame
        mask[3, 0] = False
    labels = rng.integers(1, V, size=(B, ymax + 2))
    for b in range(B):
        labels[b, :ylens[b]] = ys[b, :ylens[b]]
    return dict(logp=logp, mask=mask, ratio=ratio, labels=labels, ys=ys, ylens=ylens)


# ---------------------------------------------------------------------------------------------------------- greedy pack / row plan
PACK_CASES = ["sub", "utt_meta", "ymax_dev", "hyp_stride", "row_off", "all"]


def pack_case(kind, B=11, U=9):
    """ylen (with the EOS row, as the alignment kernel writes it) and the limit arguments of one of PACK_CASES."""
    rng = np.random.default_rng(4000 + PACK_CASES.index(kind))
    ylen = rng.integers(1, U + 1, size=B)
    ylen[0], ylen[B - 1] = U, 1
    kw = dict(U=U, hyp_stride=U + 2, sub=0, utt_meta=None, ymax=None, packed=False)
    if kind in ("sub", "all"):
        kw["sub"] = 4  # (B is no multiple of it: the last batch holds three)
    if kind == "utt_meta":
        kw["utt_meta"] = meta_of([5, 1, 5], [7, 7, 7])
        ylen[5] = 1       # a batch of one utterance without a token: one row
        ylen[6:] = np.minimum(ylen[6:], 4)
    if kind in ("ymax_dev", "all"):
        kw["ymax"] = 6
    if kind in ("hyp_stride", "all"):
        kw["hyp_stride"] = 5
    if kind in ("row_off", "all"):
        kw["packed"] = True
    if kind == "row_off":
        kw["sub"] = 3
    return ylen.astype(np.int64), kw


def pack_rows(B, U, seed=0):
    """tok (B, U) int and val (B, U) float32: the arg-max token and its log-probability per decoder row."""
    rng = np.random.default_rng(4100 + seed)
    return rng.integers(3, 40, size=(B, U)), (-rng.random((B, U)) * 3).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- collapse
COLLAPSE_TP = [1, 63, 64, 65, 130]  # one wave's 64-frame trips: short of one, exactly one, one frame of a second, a third


def collapse_case(Tp, B=7):
    rng = np.random.default_rng(5000 + Tp)
    best = rng.integers(1, 6, size=(B, Tp)) * (rng.random((B, Tp)) < 0.6)
    lens = rng.integers(1, Tp + 1, size=B)
    lens[:5] = Tp
    mask = np.arange(Tp)[None, :] < lens[:, None]
    best[0] = 0                              # all blank
    best[1] = 4                              # all the same label: one token
    best[2] = 1 + np.arange(Tp) % 2          # alternating labels: Tp tokens
    best[3] = 3                              # masked frames between equal labels: the label repeats
    mask[3, 1::3] = False
    return best.astype(np.int64), mask
