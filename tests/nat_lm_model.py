"""Plain Python / numpy restatement of the CASS-NAT finish loop with LM shallow fusion (src/models/cassnat.py:574-637 with
args.lm_weight > 0), written on the tables the device loop keeps (csrc/natlm.hip): slot s = b * beam_width + j holds one
hypothesis - tokens, the LM cache slot that produced every position (anc), the key mask (token != padding_idx), a float64 score.

``fused_row_topk`` and ``beam_step`` are the models of the two kernels; ``fused_finish`` runs the loop with them and a callable
LM, and tests/test_nat_lm_model.py pins it against the reference's own beams."""
import numpy as np


def fused_row_topk(att_row, lm_logp, lm_weight, k):
    """att_prob + lm_weight * lm_prob in float32, one rounding per operation (numpy does not contract), then the k best: sorted
    descending, ties to the lower index.  Returns (idx int32 (k,), val float32 (k,))."""
    fused = (np.asarray(att_row, np.float32) + np.float32(lm_weight) * np.asarray(lm_logp, np.float32)).astype(np.float32)
    order = np.argsort(-fused, kind="stable")[:k]
    return order.astype(np.int32), fused[order]


def init_state(B, bw, L, sos=1, pad=0):
    S = B * bw
    tok = np.full((S, L), pad, np.int32)
    tok[:, 0] = sos
    keyok = np.zeros((S, L), np.uint8)
    keyok[:, 0] = int(sos != pad)
    return dict(tok=tok, anc=np.repeat(np.arange(S, dtype=np.int32)[:, None], L, 1), keyok=keyok, score=np.zeros(S, np.float64),
                cur_tok=np.full(S, sos, np.int32))


def beam_step(st, idx, val, last, step, bw, pad=0, length_penalty=0):
    """One step of the bookkeeping (:613-636) for every utterance: candidates beam by beam, j ascending; score = parent score
    (Python float) + float(value); sorted on score + (len(hyp) - 1) * length_penalty (the score alone when None) with Python's
    stable sort; the best bw become the next beam.  One beam is live at step 0; an utterance with step > last[b] is carried."""
    S, L = st["tok"].shape
    new = {k: v.copy() for k, v in st.items()}
    for b in range(S // bw):
        if step > last[b]:
            continue
        cand = []
        for li in range(1 if step == 0 else bw):
            s = b * bw + li
            for j in range(bw):
                score = float(st["score"][s]) + float(val[s, j])
                # every candidate of this step has step + 2 tokens, sos included
                key = score + (step + 2 - 1) * length_penalty if length_penalty is not None else score
                cand.append((key, score, s, int(idx[s, j])))
        best = sorted(cand, key=lambda c: c[0], reverse=True)[:bw]
        for qn, (_, score, so, token) in enumerate(best):
            sn = b * bw + qn
            for name in ("tok", "anc", "keyok"):
                new[name][sn] = st[name][so]
            new["tok"][sn, step + 1] = token
            new["keyok"][sn, step + 1] = int(token != pad)
            new["anc"][sn, step] = so       # position `step` was computed in the parent's slot
            new["anc"][sn, step + 1] = sn   # the next one will be computed in this slot
            new["score"][sn] = score
            new["cur_tok"][sn] = token
    return new


def fused_finish(att_out, ylen, ymax, lm, beam_width, lm_weight, length_penalty, sos=1, pad=0, zero_past_len=False):
    """att_out (B, U >= ymax, V) float32 log-probabilities, ylen (B,), ``lm(ys (n, p) int64, mask (n, p, p) bool) -> (n, V)``
    log-probabilities of the LAST position.  Returns per utterance beam_width dicts (hyp, score), best first."""
    B, _, V = att_out.shape
    bw = beam_width
    last = np.minimum(np.asarray(ylen), ymax - 1)
    st = init_state(B, bw, ymax + 1, sos, pad)
    for step in range(ymax):
        ys = st["tok"][:, : step + 1].astype(np.int64)
        mask = (ys != pad)[:, None, :] & np.tril(np.ones((step + 1, step + 1), bool))[None]
        lm_logp = np.asarray(lm(ys, mask), np.float32)
        idx = np.zeros((B * bw, bw), np.int32)
        val = np.zeros((B * bw, bw), np.float32)
        for s in range(B * bw):
            b = s // bw
            row = np.zeros(V, np.float32) if zero_past_len and step >= ylen[b] else att_out[b, step]
            idx[s], val[s] = fused_row_topk(row, lm_logp[s], lm_weight, bw)
        st = beam_step(st, idx, val, last, step, bw, pad, length_penalty)
    return [[{"hyp": st["tok"][b * bw + j, : last[b] + 2].tolist(), "score": float(st["score"][b * bw + j])} for j in range(bw)]
            for b in range(B)]
