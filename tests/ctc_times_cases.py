"""The case list shared by the tests of the CTC token time stamps: every case is written out here (shapes, frame counts, labels; the
log-posteriors come from a fixed seed or are spelled out), none is sampled at run time.  Also the host entry as a function, the
sentinel-checked output buffers and the bit-for-bit comparison against tests/ctc_times_model.py."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

import ctc_times_model as tm

NEW = ["cn_op_ctc_token_times", "cn_ctc_token_times_host", "cn_ctc_token_times"]
BLANK = 0
SENT_I, SENT_F, SENT_D = -77, np.float32(-7.5), -7.25
PAD_ROWS = 2  # rows of sentinels behind the batch in every output buffer

Case = namedtuple("Case", "name logp frames labels label_len blank")
INF = float("inf")


def soft_rows(B, Tp, V, seed):
    """Random log-softmax rows: sums of them round in float32 and in float64 differently."""
    x = np.random.RandomState(seed).randn(B, Tp, V).astype(np.float32) * np.float32(2)
    m = x.max(-1, keepdims=True)
    return np.ascontiguousarray(x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True))), np.float32)


def dyadic_rows(B, Tp, V, seed):
    """Multiples of 1/4 in [-2, 0]: every sum is exact and ties are frequent."""
    return (-np.random.RandomState(seed).randint(0, 9, (B, Tp, V)) / 4.0).astype(np.float32)


def pack(name, logp, utts, extra_ld=2, blank=BLANK, frames=None, label_len=None):
    """utts: per utterance (n, labels).  ld = the longest label row + extra_ld (>= 1); unused label entries hold a sentinel id."""
    B = len(utts)
    assert logp.shape[0] == B
    ld = max(1, max(len(y) for _, y in utts) + extra_ld)
    labels = np.full((B, ld), SENT_I, np.int32)
    for b, (_, y) in enumerate(utts):
        labels[b, :len(y)] = y
    fr = np.array([n for n, _ in utts] if frames is None else frames, np.int32)
    ll = np.array([len(y) for _, y in utts] if label_len is None else label_len, np.int32)
    return Case(name, np.ascontiguousarray(logp, np.float32), fr, labels, ll, blank)


def _spelled(rows):
    """One utterance from rows written out as lists (V = len(rows[0]))."""
    return np.array([rows], np.float32)


def _cycle(L, lo=1, hi=7):
    return [lo + i % (hi - lo + 1) for i in range(L)]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # T' = 1: n 0 and 1, L 0 and 1, L > n; batch of 3 and of 1
    out.append(pack("t1_b3", soft_rows(3, 1, 8, 1), [(1, []), (0, []), (1, [3])]))
    out.append(pack("t1_b1", soft_rows(1, 1, 8, 2), [(1, [5])], extra_ld=0))
    out.append(pack("t1_more_labels_than_frames", soft_rows(3, 1, 8, 3), [(0, [3]), (1, [3, 4]), (1, [2])]))
    # T' = 2: a repeat that misses by one frame, a tight pair, n < T'
    out.append(pack("t2", soft_rows(3, 2, 8, 4), [(2, [3, 3]), (2, [3, 4]), (1, [3])]))
    # T' = 7: repeats that just fit / miss by one, L = n (tight), n < T' and n = T', soft and dyadic rows
    t7 = [(7, [1, 2, 3]), (5, [2, 2, 2]), (4, [2, 2, 2]), (7, [1, 2, 3, 4, 5, 6, 7]), (7, [1, 1, 1, 1]), (6, [1, 1, 1, 1]), (6, []), (3, [4]),
          (7, [5, 5, 2, 2])]
    out.append(pack("t7_soft", soft_rows(len(t7), 7, 8, 5), t7))
    out.append(pack("t7_dyadic", dyadic_rows(len(t7), 7, 8, 6), t7, extra_ld=4))
    out.append(pack("t7_dyadic_b", dyadic_rows(len(t7), 7, 8, 7), t7, extra_ld=1))
    # T' = 40, V = 5000, a ragged batch of 33: n from 40 down to 8, L 0 .. 8 and one tight row, repeats inside
    t40 = [(40 - b, ([7 + 13 * b, 7 + 13 * b] + _cycle(b % 9, 100 + b, 4000))[: (b % 9)]) for b in range(33)]
    t40[5] = (35, _cycle(35, 10, 4999))  # tight: L = n
    t40[6] = (34, [])
    out.append(pack("t40_v5000_b33", soft_rows(33, 40, 5000, 8), t40))
    # T' = 300: L = 150 (S = 301 states, wider than the workgroup) loose and tight, with repeats that just fit, and a single label
    t300 = [(300, _cycle(150)), (150, _cycle(150)), (300, [3] * 150), (299, [3] * 150), (298, [3] * 150), (300, [4]), (17, _cycle(9))]
    out.append(pack("t300_v8", soft_rows(len(t300), 300, 8, 9), t300, extra_ld=3))
    out.append(pack("t300_dyadic", dyadic_rows(3, 300, 8, 10), [(300, _cycle(150)), (300, [3] * 150), (211, _cycle(70))]))
    out.append(pack("t300_v5000_b1", soft_rows(1, 300, 5000, 11), [(300, _cycle(40, 1, 4999))]))
    # T' = 3000: the back-pointers of 3000 frames x 2 chunks do not fit the launch's LDS, the default takes the scratch form
    out.append(pack("t3000_past_the_lds", soft_rows(2, 3000, 8, 18), [(3000, _cycle(40)), (1500, [3] * 40)]))
    # bad labels in one utterance of a batch: the blank, V, a negative id, a huge id; the neighbours are unaffected
    out.append(pack("bad_blank", soft_rows(3, 7, 8, 12), [(7, [1, 2]), (7, [1, BLANK, 2]), (7, [3, 4])]))
    out.append(pack("bad_range", soft_rows(4, 7, 8, 13), [(7, [8]), (7, [1, 2]), (7, [2, -1]), (7, [1 << 30, 1])]))
    out.append(pack("bad_v5000", soft_rows(3, 40, 5000, 14), [(40, [4999, 1]), (40, [5000]), (40, [17, 17, 4999])]))
    # counts outside their ranges are clamped: frames > T' and < 0, label_len > ld and < 0
    out.append(pack("clamped", soft_rows(4, 7, 8, 15), [(7, [1, 2, 3]), (0, [1, 2, 3]), (7, [4, 5, 6]), (7, [])], extra_ld=0,
                    frames=[9, -2, 7, 7], label_len=[3, 3, 5, -4]))
    # a blank that is not id 0
    out.append(pack("blank_5", soft_rows(2, 7, 8, 16), [(7, [0, 1, 0]), (7, [5])], blank=5))
    # ---- ties, spelled out (V = 4, multiples of 1/4) ----
    zero = [[0.0] * 4] * 5
    # every path ties: stay beats s-1 beats s-2 at every frame, and the last label beats the trailing blank at the end
    out.append(pack("tie_all_zero", np.concatenate([_spelled(zero)] * 3), [(5, [1, 2]), (3, [1]), (5, [2, 2])]))
    # state 3 at frame 2: stay is worse (-1), s-1 and s-2 tie (0): s-1 wins
    out.append(pack("tie_s1_vs_s2", _spelled([[0, 0, 0, 0], [0, 0, -1, 0], [0, 0, 0, 0]]), [(3, [1, 2])]))
    # state 1 at frame 1: stay (0) ties s-1 from the blank (0): stay wins, label 1 starts at frame 0
    out.append(pack("tie_stay_vs_s1", _spelled([[0, 0, 0, 0], [-0.25, 0, 0, 0], [-0.5, -0.25, 0, 0]]), [(3, [1])]))
    # the end: a[2L-1] == a[2L] exactly, with unequal rows in front
    out.append(pack("tie_end", _spelled([[-0.5, -0.25, 0, 0], [-0.75, -0.5, 0, 0], [-0.25, -0.25, 0, 0]]), [(3, [1])]))
    # the blank between equal labels cannot be skipped although skipping it scores better
    out.append(pack("no_skip_between_equal", _spelled([[-2, 0, 0, 0]] * 3 + [[-2, 0, -1, 0]]), [(3, [1, 1])], frames=[3]))
    # ---- rows holding -inf ----
    inf = soft_rows(4, 7, 8, 17)
    inf[0, 2, 1] = inf[0, 3, BLANK] = -INF          # a finite path remains
    inf[1, :, 2] = -INF
    inf[1, 4, 2] = np.float32(-0.5)                 # label 2 is possible at frame 4 only
    inf[2, 0, :] = -INF                             # every path has probability zero: score -inf, spans by the tie rules
    inf[3, :, 3] = -INF                             # label 3 never possible
    out.append(pack("minus_inf", inf, [(7, [1, 2]), (7, [1, 2, 3]), (7, [1, 2]), (6, [3])]))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The model's answer, computed once per case."""
    c = case(name)
    return tm.align_batch(c.logp, c.frames, c.labels, c.label_len, c.blank)


def out_buffers(c):
    """start, end, conf, score, status with PAD_ROWS rows of sentinels behind the batch (numpy; the GPU tests copy them up)."""
    B, ld = c.labels.shape
    return (np.full((B + PAD_ROWS, ld), SENT_I, np.int32), np.full((B + PAD_ROWS, ld), SENT_I, np.int32),
            np.full((B + PAD_ROWS, ld), SENT_F, np.float32), np.full(B + PAD_ROWS, SENT_D, np.float64), np.full(B + PAD_ROWS, SENT_I, np.int32))


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def run_host(c, lib=None):
    from cassnat_asr_public_amd import hip

    L = lib or hip.lib()
    B, Tp, V = c.logp.shape
    start, end, conf, score, status = out_buffers(c)
    rc = L.cn_ctc_token_times_host(p(c.logp), p(c.frames), p(c.labels), c.labels.shape[1], p(c.label_len), B, Tp, V, c.blank, -1, p(start), p(end),
                                   p(conf), p(score), p(status))
    assert rc == 0, L.cn_last_error()
    return start, end, conf, score, status


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.int32, 8: np.int64}[x.dtype.itemsize])


def same_as_model(c, got, want=None):
    """Integers, conf and score bit for bit; nothing written past a row's labels or past the batch."""
    start, end, conf, score, status = got
    want = expected(c.name) if want is None else want
    B, ld = c.labels.shape
    for b, w in enumerate(want):
        L = len(w["start"])
        where = (c.name, b)
        assert int(status[b]) == w["status"], where
        assert start[b, :L].tolist() == w["start"] and end[b, :L].tolist() == w["end"], (where, start[b, :L].tolist(), end[b, :L].tolist(), w)
        assert np.array_equal(bits(conf[b, :L]), bits(w["conf"])), (where, conf[b, :L], w["conf"])
        assert bits(np.float64(score[b])) == bits(np.float64(w["score"])), (where, float(score[b]), w["score"])
        assert (start[b, L:] == SENT_I).all() and (end[b, L:] == SENT_I).all() and (conf[b, L:] == SENT_F).all(), where
    assert (start[B:] == SENT_I).all() and (end[B:] == SENT_I).all() and (conf[B:] == SENT_F).all(), c.name
    assert (score[B:] == SENT_D).all() and (status[B:] == SENT_I).all(), c.name
