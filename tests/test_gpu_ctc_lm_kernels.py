"""The kernels of the CTC prefix beam search with the LM in the frame loop (csrc/ctc_lm.hip, and the LM step with a position per
row in csrc/ast.hip) one at a time, through cn_op_ctc_lm_frame, cn_op_ctc_lm_rows and cn_lm_step_rows, against
tests/ctc_lm_model.py (which tests/test_ctc_lm_model.py pins to the reference's beams).  Integers, order and tables are exact,
float64 scores within 1e-8 (the figure of tests/test_gpu_ctcbeam.py for the LM-free kernel); LM rows equal cn_lm_step's."""
import ctypes as C

import numpy as np
import pytest
import torch

from cassnat_asr_public_amd import hip, synth
from cassnat_asr_public_amd.models.lm import make_model as make_lm
from ctc_lm_model import LOGZERO, frame_step, init_state

pytestmark = pytest.mark.gpu

SOS, BLANK = 1, 0


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Frame:
    """Device arrays of cn_op_ctc_lm_frame for B utterances of W slots, and the call."""

    def __init__(self, B, W, Lt, hist):
        S = B * W
        self.B, self.W, self.Lt, self.hist = B, W, Lt, hist
        self.f64 = {k: torch.full((S,), LOGZERO, dtype=torch.float64, device="cuda") for k in ("pb", "pnb", "sctc", "slm")}
        self.i32 = {k: torch.full((S,), -5, dtype=torch.int32, device="cuda") for k in ("len", "last", "tok", "pos", "parent", "stay")}
        self.nb = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.rowid = [torch.full((S, Lt), -9, dtype=torch.int32, device="cuda") for _ in range(2)]
        self.hpar = torch.full((B, hist, W), 255, dtype=torch.uint8, device="cuda")
        self.htok = torch.full((B, hist, W), -7, dtype=torch.int32, device="cuda")

    def put(self, b, st, rowids=None):
        """The kept hypotheses of utterance b (ctc_lm_model state) into its slots."""
        n, s0 = len(st["pb"]), b * self.W
        for k in ("pb", "pnb", "sctc", "slm"):
            self.f64[k][s0:s0 + n] = dev(np.asarray(st[k], np.float64))
        for k in ("len", "last"):
            self.i32[k][s0:s0 + n] = dev(np.asarray(st[k], np.int32))
        self.nb[b] = n
        if rowids is not None:
            self.rowid[self.cur][s0:s0 + n] = dev(rowids.astype(np.int32))

    cur = 0

    def step(self, it, logp, top, lmrow, frames, count, P, lp, w):
        self.cur = it & 1
        B, Tp, V = logp.shape
        a = self
        rc = hip.lib().cn_op_ctc_lm_frame(p(a.f64["pb"]), p(a.f64["pnb"]), p(a.f64["sctc"]), p(a.f64["slm"]), p(a.i32["len"]), p(a.i32["last"]),
                                          p(a.nb), p(a.i32["tok"]), p(a.i32["pos"]), p(a.i32["parent"]), p(a.i32["stay"]),
                                          p(a.rowid[it & 1]), p(a.rowid[(it & 1) ^ 1]), p(a.hpar), p(a.htok), p(logp), p(top), p(lmrow),
                                          p(frames), p(count), B, Tp, V, a.W, P, BLANK, SOS, it, a.Lt, a.hist, float(lp), float(w),
                                          hip.current_stream())
        hip.check(rc, "cn_op_ctc_lm_frame")
        torch.cuda.synchronize()

    def get(self, b):
        s0, n = b * self.W, int(self.nb[b])
        out = {k: v[s0:s0 + self.W].cpu().numpy() for k, v in {**self.f64, **self.i32}.items()}
        out["n"] = n
        out["rowid"] = self.rowid[self.cur ^ 1][s0:s0 + self.W].cpu().numpy()
        return out


def make_inputs(g, B, Tp, V, P, W, ties):
    """Log-posteriors and LM rows; ``ties``: both on a coarse grid with repeated values and LM zeros, so that candidates of one
    hypothesis tie exactly (same CTC term, a zero LM term) and list order must decide."""
    logits = g.standard_normal((B, Tp, V)).astype(np.float32) * 2
    if ties:
        logits = np.round(logits)
    logp = torch.log_softmax(torch.from_numpy(logits), -1).numpy()
    if ties:  # equal log-posteriors for groups of labels
        logp[:, :, 4:8] = logp[:, :, 4:5]
    lm = torch.log_softmax(torch.from_numpy(g.standard_normal((B * W, V)).astype(np.float32) * 2), -1).numpy()
    if ties:
        lm[:, 4:8] = 0.0
    top = torch.topk(torch.from_numpy(logp), P, dim=-1)[1].numpy().astype(np.int32) if P > 0 else np.zeros((B, Tp, 1), np.int32)
    return logp, lm, top


def check_utt(got, want, parent, tok, old_len, old_rowid, it, S, s0, W):
    n = len(parent)
    assert got["n"] == n
    for k in ("pb", "pnb", "sctc", "slm"):
        np.testing.assert_allclose(got[k][:n], want[k], rtol=0, atol=1e-8, err_msg=k)
    assert got["len"][:n].tolist() == want["len"].tolist() and got["last"][:n].tolist() == want["last"].tolist()
    assert got["parent"][:n].tolist() == (parent + s0).tolist()
    assert got["stay"][:n].tolist() == (tok < 0).astype(int).tolist()
    assert got["pos"][:n].tolist() == want["len"].tolist()
    assert got["tok"][:n].tolist() == [int(l) if l >= 0 else SOS for l in want["last"]]
    # unused slots: carried dummies that ask nothing of the LM step
    assert got["stay"][n:].tolist() == [1] * (W - n) and got["pos"][n:].tolist() == [0] * (W - n) and got["tok"][n:].tolist() == [SOS] * (W - n)
    for r in range(n):
        pl = int(old_len[parent[r]])
        assert got["rowid"][r, : pl + 1].tolist() == old_rowid[parent[r], : pl + 1].tolist(), r
        if tok[r] >= 0:
            assert got["rowid"][r, pl + 1] == (it + 1) * S + s0 + r


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("W,P", [(1, 1), (5, 8), (20, 30), (32, 32), (7, 0)])
def test_frame_kernel_chain_from_the_initial_state(W, P, ties):
    """Six iterations from the initial state: the live count grows from 1 towards W; utterance 1 ends after two iterations and
    utterance 2 has no frame at all (both stand from then on); the blank sits inside the pruned lists; a kept hypothesis' last label
    is among the pruned labels (repetition); with ``ties`` many keys are exactly equal."""
    B, Tp, V, K = 4, 9, 40, 6
    g = np.random.default_rng(W * 100 + P + ties)
    count = np.array([K, 2, 0, K], np.int32)
    frames = np.stack([np.sort(g.choice(Tp, K, replace=False)) for _ in range(B)]).astype(np.int32)
    frames = np.concatenate([frames, np.zeros((B, Tp - K), np.int32)], 1)
    fr = Frame(B, W, K + 2, K)
    states = [init_state() for _ in range(B)]
    rowids = [np.full((W, K + 2), -9, np.int64) for _ in range(B)]
    for b in range(B):
        rowids[b][:, 0] = b * W + np.arange(W)
        fr.put(b, states[b], rowids[b][:1])
    frames_d, count_d = dev(frames), dev(count)
    saw_blank = saw_rep = False
    for it in range(K):
        logp, lm, top = make_inputs(g, B, Tp, V, P, W, ties)
        if P > 1:
            top[:, :, 1] = BLANK  # the blank inside every pruned list
        for b in range(B):  # the best hypothesis' last label first in the list: a repetition among the candidates
            if P > 0 and it < count[b] and states[b]["last"][0] >= 0:
                top[b, frames[b, it], 0] = states[b]["last"][0]
        logp_d, lm_d, top_d = dev(logp), dev(lm), dev(top)
        before = [fr.get(b) for b in range(B)]
        fr.step(it, logp_d, top_d, lm_d, frames_d, count_d, P, 0.2, 0.3)
        for b in range(B):
            got = fr.get(b)
            if it >= count[b]:
                for k in ("pb", "pnb", "sctc", "slm", "len", "last"):
                    assert np.array_equal(got[k], before[b][k]), (b, k)
                assert got["n"] == before[b]["n"] and got["stay"].tolist() == [1] * W
                continue
            t = frames[b, it]
            st = states[b]
            n_old = len(st["pb"])
            tp = top[b, t, :P]
            saw_blank |= BLANK in tp.tolist()
            saw_rep |= any(int(l) in tp.tolist() for l in st["last"] if l >= 0)
            new, parent, tok = frame_step(st, logp[b, t], tp, lm[b * W: b * W + n_old], W, 0.2, 0.3)
            check_utt(got, new, parent, tok, st["len"], rowids[b], it, B * W, b * W, W)
            nr = np.full_like(rowids[b], -9)
            for r in range(len(parent)):
                pl = int(st["len"][parent[r]])
                nr[r, : pl + 1] = rowids[b][parent[r], : pl + 1]
                if tok[r] >= 0:
                    nr[r, pl + 1] = (it + 1) * B * W + b * W + r
            assert fr.hpar[b, it, : len(parent)].cpu().tolist() == parent.tolist()
            assert fr.htok[b, it, : len(parent)].cpu().tolist() == tok.tolist()
            # the next step of the model runs on the DEVICE's float64 state (within 1e-8 of its own): no drift between the two chains
            for k in ("pb", "pnb", "sctc", "slm"):
                new[k] = got[k][: len(parent)].astype(np.float64)
            states[b], rowids[b] = new, nr
    assert saw_blank == (P > 1) and (saw_rep or P <= 1)
    assert len(states[0]["pb"]) == (W if P > 1 else 1 if P == 0 else len(states[0]["pb"]))


@pytest.mark.parametrize("W,P", [(1, 1), (5, 8), (20, 30), (32, 32)])
def test_frame_kernel_on_random_states(W, P):
    """One step on random kept hypotheses: live counts 0, 1, W // 2 + 1 and W; lengths 0 .. iter with last labels to match."""
    B, Tp, V, it = 4, 6, 40, 5
    g = np.random.default_rng(7 * W + P)
    live = [0, 1, min(W, W // 2 + 1), W]
    logp, lm, top = make_inputs(g, B, Tp, V, P, W, False)
    if P > 2:
        top[:, :, 2] = BLANK
    frames = np.tile(np.arange(Tp, dtype=np.int32)[::-1], (B, 1)).copy()
    count = np.full(B, Tp, np.int32)
    fr = Frame(B, W, it + 2, it + 1)
    fr.cur = it & 1
    states, rowids = [], []
    for b, n in enumerate(live):
        ln = g.integers(0, it + 1, n)
        last = np.where(ln > 0, g.integers(1, V, n), -1)
        if n > 1 and P > 0:
            ln[1], last[1] = 2, top[b, frames[b, it], 0]  # a repetition of the last label among the candidates
        pb, pnb = -g.random(n) * 5, -g.random(n) * 5
        pnb = np.where(ln > 0, pnb, LOGZERO)
        st = dict(pb=pb, pnb=pnb, sctc=np.logaddexp(pb, pnb), slm=-g.random(n) * 3, len=ln.astype(np.int64), last=last.astype(np.int64))
        rid = g.integers(0, (it + 1) * B * W, (n, it + 2))
        states.append(st)
        rowids.append(rid)
        fr.put(b, st, rid)
    fr.step(it, dev(logp), dev(top), dev(lm), dev(frames), dev(count), P, 0.1, 0.7)
    for b, n in enumerate(live):
        t = frames[b, it]
        new, parent, tok = frame_step(states[b], logp[b, t], top[b, t, :P], lm[b * W: b * W + n], W, 0.1, 0.7)
        check_utt(fr.get(b), new, parent, tok, states[b]["len"], rowids[b], it, B * W, b * W, W)
    assert fr.get(0)["n"] == 0


@pytest.mark.parametrize("V", [40, 5000, 1027])
def test_rows_kernel_copies_the_parent_row_or_takes_the_fresh_one(V):
    B, W = 3, 5
    S = B * W
    g = np.random.default_rng(V)
    fresh, prv = g.standard_normal((S, V)).astype(np.float32), g.standard_normal((S, V)).astype(np.float32)
    parent = np.concatenate([b * W + g.integers(0, W, W) for b in range(B)]).astype(np.int32)
    stay = g.integers(0, 2, S).astype(np.int32)
    count = np.array([9, 2, 3], np.int32)  # iteration 2: utterance 1 has ended
    nxt = torch.full((S, V), 77.0, device="cuda")
    f_d, p_d, par_d, stay_d, cnt_d = dev(fresh), dev(prv), dev(parent), dev(stay), dev(count)
    hip.check(hip.lib().cn_op_ctc_lm_rows(p(f_d), p(p_d), p(nxt), p(par_d), p(stay_d), p(cnt_d), 2, S, W, V, hip.current_stream()))
    torch.cuda.synchronize()
    got = nxt.cpu().numpy()
    for s in range(S):
        want = np.full(V, 77.0, np.float32) if s // W == 1 else (prv[parent[s]] if stay[s] else fresh[s])
        assert np.array_equal(got[s], want), s
    hip.check(hip.lib().cn_op_ctc_lm_rows(p(f_d), p(p_d), p(nxt), p(par_d), p(stay_d), None, 2, S, W, V, hip.current_stream()))
    torch.cuda.synchronize()
    assert np.array_equal(nxt.cpu().numpy()[W], prv[parent[W]] if stay[W] else fresh[W])  # without count nothing is skipped


# ------------------------------------------------------------------------------------------- the LM step with a position per row
def lm_engine(prec, slots, max_len):
    lm_args = synth.make_args_lm("tiny_lm", vocab_size=40)
    lm_args.hip_precision = prec
    lm = make_lm(lm_args).cuda()
    with torch.no_grad():
        for k, q in lm.named_parameters():
            q.copy_(torch.from_numpy(synth.make_state(lm_args, seed=9, gain=2.0)[k]))
    eng = lm.step_engine(slots)
    eng.lm_step_begin(max_len, slots)
    return lm, eng


def scratch_rows(eng, prefixes, n):
    """log-probability row after the last token of every prefix, by cn_lm_step from position 0 on n rows at a time (the rows of one
    call share a length; a short group is filled up with copies of its first prefix)."""
    V, out = 40, {}
    for L in sorted(set(len(q) for q in prefixes)):
        group = [q for q in dict.fromkeys(map(tuple, prefixes)) if len(q) == L]
        for c0 in range(0, len(group), n):
            chunk = group[c0:c0 + n]
            rows = chunk + [chunk[0]] * (n - len(chunk))
            anc = dev(np.tile(np.arange(n, dtype=np.int32)[:, None], (1, L)))
            keyok = torch.ones(n, L, dtype=torch.uint8, device="cuda")
            logp = torch.empty(n, V, device="cuda")
            for pos in range(L):
                eng.lm_step(pos, dev(np.array([r[pos] for r in rows], np.int32)), anc, keyok, logp)
            torch.cuda.synchronize()
            for i, q in enumerate(chunk):
                out[q] = logp[i].cpu().numpy().copy()
    return out


class RowTables:
    """The row-id rule of the frame kernel, restated: a slot's ids are its parent's, plus iteration * S + slot for a new label."""

    def __init__(self, S, Lt):
        self.S, self.Lt = S, Lt
        self.hyp = [[SOS] for _ in range(S)]
        self.ids = [[s] for s in range(S)]
        self.stay = [0] * S
        self.it = 0

    def advance(self, moves):
        """moves[s] = (parent slot, appended token or None)"""
        self.it += 1
        hyp, ids, stay = [], [], []
        for s, (par, tok) in enumerate(moves):
            hyp.append(self.hyp[par] + ([tok] if tok is not None else []))
            ids.append(self.ids[par] + ([self.it * self.S + s] if tok is not None else []))
            stay.append(int(tok is None))
        self.hyp, self.ids, self.stay = hyp, ids, stay

    def run(self, eng):
        S, V = self.S, 40
        rid = np.zeros((S, self.Lt), np.int32)
        for s in range(S):
            rid[s, : len(self.ids[s])] = self.ids[s]
        logp = torch.full((S, V), 55.0, device="cuda")
        pos = np.array([len(h) - 1 for h in self.hyp], np.int32)
        eng.lm_step_rows(int(pos.max()), dev(np.array([h[-1] for h in self.hyp], np.int32)), dev(pos), dev(np.array(self.stay, np.int32)),
                         dev(rid), logp)
        torch.cuda.synchronize()
        return logp.cpu().numpy()


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16"])
def test_lm_step_with_a_position_per_row_equals_cn_lm_step_per_length(prec):
    """Six hypotheses of lengths 1 .. 5 grow side by side, each by its own schedule (some wait - 'stay' - while others append):
    every fresh row is cn_lm_step's row for that prefix, run from position 0 on rows of one length."""
    S = 6
    lm, eng = lm_engine(prec, S, 8)
    g = np.random.default_rng(1)
    target = [g.integers(4, 40, n).tolist() for n in (1, 2, 3, 3, 5, 4)]
    tb = RowTables(S, 8)
    fresh = {}
    out = tb.run(eng)
    for s in range(S):
        fresh[tuple(tb.hyp[s])] = out[s]
    done = [0] * S
    for it in range(7):
        moves = []
        for s in range(S):
            go = done[s] < len(target[s]) and (it + s) % 3 != 0  # every slot waits now and then
            moves.append((s, target[s][done[s]] if go else None))
            done[s] += go
        tb.advance(moves)
        out = tb.run(eng)
        for s in range(S):
            if not tb.stay[s]:
                fresh[tuple(tb.hyp[s])] = out[s]
    assert all(d == len(t) for d, t in zip(done, target))
    assert len(set(len(k) for k in fresh)) >= 5
    want = scratch_rows(eng, list(fresh), S)
    for q, row in fresh.items():
        assert np.array_equal(row, want[q]), (q, float(np.abs(row - want[q]).max()))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_a_reoccupied_slot_never_rewrites_a_row_a_descendant_reads(prec):
    """The cache hazard: slot 2 computes position 3 of [7, 10, 13]; its children move to slots 0 and 1; slot 2 is taken by the empty
    hypothesis, which grows to three labels again - under (position, slot) addressing it would overwrite the key and value its
    cousins still read.  Every fresh row, the cousins' last ones included, equals the LM run from scratch on its prefix."""
    S = 4
    lm, eng = lm_engine(prec, S, 10)
    tb = RowTables(S, 10)
    seq = [
        [(0, 5), (0, 6), (1, 7), (3, None)],
        [(0, 8), (1, 9), (2, 10), (3, None)],
        [(2, 11), (2, 12), (2, 13), (3, None)],       # slot 2: [7, 10, 13], position 3 computed in slot 2
        [(2, 14), (2, 15), (3, None), (3, 16)],       # its children in slots 0 and 1; slot 2 reoccupied by the empty hypothesis
        [(0, None), (1, None), (2, 17), (3, 18)],
        [(0, None), (1, None), (2, 19), (3, None)],
        [(0, None), (1, None), (2, 20), (3, None)],   # slot 2 is at position 3 again
        [(0, 21), (1, 22), (2, None), (3, None)],     # the cousins read position 3 of THEIR prefix
    ]
    fresh = {}
    out = tb.run(eng)
    fresh[(SOS,)] = out[0]
    for moves in seq:
        tb.advance(moves)
        out = tb.run(eng)
        for s in range(S):
            if not tb.stay[s]:
                fresh[tuple(tb.hyp[s])] = out[s]
    assert tb.hyp[0] == [SOS, 7, 10, 13, 14, 21] and tb.hyp[1] == [SOS, 7, 10, 13, 15, 22] and tb.hyp[2] == [SOS, 17, 19, 20]
    assert tb.ids[0][3] == tb.ids[1][3] == 3 * S + 2 and tb.ids[2][3] == 7 * S + 2  # same (position, slot), two different rows
    want = scratch_rows(eng, list(fresh), S)
    for q, row in fresh.items():
        assert np.array_equal(row, want[q]), (q, float(np.abs(row - want[q]).max()))


def test_kernel_entries_refuse_bad_arguments_before_a_launch():
    L = hip.lib()
    B, W, Tp, V, P, Lt = 2, 3, 4, 40, 5, 6
    fr = Frame(B, W, Lt, 4)
    logp, top, lm = torch.zeros(B, Tp, V, device="cuda"), torch.zeros(B, Tp, P, dtype=torch.int32, device="cuda"), torch.zeros(B * W, V, device="cuda")
    frames, count = torch.zeros(B, Tp, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")

    def call(W_=W, P_=P, it=0, Lt_=Lt, hist=4, blank=0, sos=1, top_=top):
        a = fr
        return L.cn_op_ctc_lm_frame(p(a.f64["pb"]), p(a.f64["pnb"]), p(a.f64["sctc"]), p(a.f64["slm"]), p(a.i32["len"]), p(a.i32["last"]),
                                    p(a.nb), p(a.i32["tok"]), p(a.i32["pos"]), p(a.i32["parent"]), p(a.i32["stay"]), p(a.rowid[0]),
                                    p(a.rowid[1]), p(a.hpar), p(a.htok), p(logp), p(top_), p(lm), p(frames), p(count), B, Tp, V, W_, P_,
                                    blank, sos, it, Lt_, hist, 0.0, 0.3, hip.current_stream())

    for kw, msg in ((dict(W_=33), b"ctc_beam <= 32"), (dict(W_=0), b"ctc_beam <= 32"), (dict(P_=33), b"ctc_pruning <= 32"),
                    (dict(it=4), b"iteration outside"), (dict(it=-1), b"iteration outside"), (dict(Lt_=1), b"iteration outside"),
                    (dict(blank=40), b"blank outside"), (dict(sos=40), b"sos inside"), (dict(top_=None), b"null array")):
        assert call(**kw) != 0, kw
        assert msg in L.cn_last_error(), (kw, L.cn_last_error())
    assert L.cn_op_ctc_lm_rows(p(lm), p(lm), None, p(count), p(count), None, 0, B * W, W, V, hip.current_stream()) != 0
    assert b"null array" in L.cn_last_error()
    assert L.cn_op_ctc_lm_rows(p(lm), p(lm), p(lm), p(count), p(count), None, 0, B * W + 1, W, V, hip.current_stream()) != 0
    assert b"slots = B * ctc_beam" in L.cn_last_error()
    torch.cuda.synchronize()
    assert call() == 0  # the same buffers with a valid geometry are accepted (count 0: nothing but the stay flags is written)
    torch.cuda.synchronize()
    lm_, eng = lm_engine("fp32", 4, 4)
    t = torch.zeros(4, dtype=torch.int32, device="cuda")
    rid = torch.zeros(4, 4, dtype=torch.int32, device="cuda")
    out = torch.zeros(4, 40, device="cuda")
    for kw in (dict(n=5), dict(max_pos=4), dict(max_pos=-1), dict(stride=2, max_pos=2)):
        n, mp, stride = kw.get("n", 4), kw.get("max_pos", 0), kw.get("stride", 4)
        assert eng.L.cn_lm_step_rows(eng.handle, n, mp, p(t), p(t), p(t), p(rid), stride, p(out), hip.current_stream()) != 0, kw
        assert b"outside the configured cache" in eng.L.cn_last_error()
    assert eng.L.cn_lm_step_rows(eng.handle, 4, 0, p(t), None, p(t), p(rid), 4, p(out), hip.current_stream()) != 0
    assert b"null array" in eng.L.cn_last_error()
