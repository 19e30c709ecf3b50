"""The yardstick of the CTC token time stamps (include/cassnat_hip_ctc_times.h): a forced alignment of given labels over float32
log-posteriors in float64 with true -inf, spans and confidences per label.  Plain Python floats (IEEE double), no torch, no library.

``align`` is the definition.  ``MISTAKES`` names six deliberate errors ``align(..., mistake=name)`` can make; the tests check that every
one of them is caught by the shared case list.  ``brute`` enumerates every path of a small case."""
import itertools
import math

import numpy as np

NINF = -math.inf
MISTAKES = ("tie_order", "skip_equal", "end_tie", "float32", "blank_span", "conf_mean")


def clamp(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def feasible_by_count(labels, n):
    """A path exists iff every label and every blank between two equal labels gets a frame of its own."""
    labels = list(labels)
    return len(labels) + sum(1 for i in range(1, len(labels)) if labels[i] == labels[i - 1]) <= n


def status_of(labels, n, V, blank):
    if any(y < 0 or y >= V or y == blank for y in labels):
        return 2
    return 0 if feasible_by_count(labels, n) else 1


def _add(a, b, f32):
    return float(np.float32(a) + np.float32(b)) if f32 else a + b


def align(lp, n, labels, blank, mistake=None):
    """lp (T', V) float32, n valid frames, labels a sequence of ints -> dict(status, start, end, conf (float32), score (float))."""
    assert mistake is None or mistake in MISTAKES
    lp = np.asarray(lp, np.float32)
    Tp, V = lp.shape
    n = clamp(int(n), 0, Tp)
    labels = [int(y) for y in labels]
    L = len(labels)
    out = dict(status=status_of(labels, n, V, blank), start=[-1] * L, end=[-1] * L, conf=np.zeros(L, np.float32), score=NINF)
    if out["status"] != 0:
        return out
    if n == 0:  # (then L == 0: the empty path)
        out["score"] = 0.0
        return out
    S = 2 * L + 1
    path = [blank] * S
    path[1::2] = labels
    f32 = mistake == "float32"
    a = [NINF] * S
    for s in range(min(S, 2)):
        a[s] = float(lp[0, path[s]])
    bp = []
    for t in range(1, n):
        nxt, mv = [NINF] * S, [0] * S
        for s in range(S):
            cands = [(a[s], 0)]
            if s >= 1:
                cands.append((a[s - 1], 1))
            if (s & 1) and s >= 3 and (path[s - 2] != path[s] or mistake == "skip_equal"):
                cands.append((a[s - 2], 2))
            if mistake == "tie_order":
                cands.reverse()
            best, move = cands[0]
            for v, m in cands[1:]:  # the first of the list wins a tie
                if v > best:
                    best, move = v, m
            nxt[s], mv[s] = _add(best, float(lp[t, path[s]]), f32), move
        a = nxt
        bp.append(mv)
    if L == 0:
        cur = 0
    elif mistake == "end_tie":
        cur = 2 * L - 1 if a[2 * L - 1] > a[2 * L] else 2 * L
    else:
        cur = 2 * L - 1 if a[2 * L - 1] >= a[2 * L] else 2 * L
    out["score"] = a[cur]
    states = [cur]
    for t in range(n - 1, 0, -1):
        cur -= bp[t - 1][cur]
        states.append(cur)
    states.reverse()
    return _spans(out, lp, states, labels, mistake)


def _spans(out, lp, states, labels, mistake=None):
    for u, y in enumerate(labels):
        want = 2 * u + (2 if mistake == "blank_span" else 1)
        frames = [t for t, s in enumerate(states) if s == want]
        if not frames:
            continue
        out["start"][u], out["end"][u] = frames[0], frames[-1] + 1
        vals = lp[frames[0]:frames[-1] + 1, y]
        out["conf"][u] = np.float32(vals.astype(np.float64).mean()) if mistake == "conf_mean" else vals.max()
    return out


def brute(lp, n, labels, blank):
    """Every path of a small case: the best score as the sequential float64 sum in frame order, and among the paths that reach it the
    one the tie rules name - the last label's state before the trailing blank at the end, then, frame by frame backwards, the highest
    state (stay before s-1 before s-2).  Returns ``align``'s dict; status 1 exactly when no path was found."""
    lp = np.asarray(lp, np.float32)
    labels = [int(y) for y in labels]
    L, S = len(labels), 2 * len(labels) + 1
    out = dict(status=0, start=[-1] * L, end=[-1] * L, conf=np.zeros(L, np.float32), score=NINF)
    if n == 0:
        out["status"], out["score"] = (0, 0.0) if L == 0 else (1, NINF)
        return out
    path = [blank] * S
    path[1::2] = labels
    best = None
    for states in itertools.product(range(S), repeat=n):
        if states[0] > 1 or states[-1] not in ((0,) if L == 0 else (2 * L - 1, 2 * L)):
            continue
        ok = True
        for p, s in zip(states, states[1:]):
            d = s - p
            if d < 0 or d > 2 or (d == 2 and (not (s & 1) or path[p] == path[s])):
                ok = False
                break
        if not ok:
            continue
        score = float(lp[0, path[states[0]]])
        for t in range(1, n):
            score = score + float(lp[t, path[states[t]]])
        key = (score, states[-1] == 2 * L - 1) + tuple(reversed(states[:-1]))
        if best is None or key > best[0]:
            best = (key, states)
    if best is None:
        out["status"] = 1
        return out
    out["score"] = best[0][0]
    return _spans(out, lp, list(best[1]), labels)


def align_batch(logp, frames, labels, label_len, blank, mistake=None):
    """The entries' layout: logp (B, T', V), frames (B,), labels (B, ld), label_len (B,) -> per utterance ``align``'s dict
    (label_len clamped to [0, ld])."""
    ld = labels.shape[1]
    return [align(logp[b], frames[b], labels[b, :clamp(int(label_len[b]), 0, ld)], blank, mistake) for b in range(logp.shape[0])]
