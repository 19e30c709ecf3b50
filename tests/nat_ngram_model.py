"""numpy restatement of the CASS-NAT finish loop with word n-gram fusion (include/cassnat_hip_nat_ngram.h), over full vocabulary rows.
Nothing here comes from the code under test: the adds of a hypothesis are ast_ngram_model.adds (the words ctc_ngram_model finds, the
scores WordModel's), the beam bookkeeping is nat_lm_model.beam_step (which tests/test_nat_lm_model.py pins to the reference's beams).

A slot's candidates at step i are the beam_width best of fused(c) = fl32(att[b][i][c] + fl32(lm_scale * term(c))) over the whole
vocabulary, ordered by (fused descending, att descending, index ascending); ``slot_topk`` is that definition, ``class_tables`` and
``slot_topk_from_tables`` the form the device computes it in (tests/test_nat_ngram_model.py holds the two against each other)."""
import numpy as np

import ast_ngram_model as model_of
from nat_lm_model import beam_step, init_state

F32 = np.float32


def term_row(adds, starts, eos):
    """The term of every candidate of the vocabulary for a hypothesis with adds (a_word, a_eos): float32 (V,)."""
    t = np.where(np.asarray(starts) != 0, F32(adds[0]), F32(0.0)).astype(F32)
    t[eos] = F32(adds[1])
    return t


def fuse(att, scale, term):
    """fl32(att + fl32(scale * term)), one rounding per operation (numpy does not contract)."""
    return (np.asarray(att, F32) + (F32(scale) * np.asarray(term, F32)).astype(F32)).astype(F32)


def _order(fused, att, idx):
    """Positions sorted by (fused descending, att descending, index ascending)."""
    return np.lexsort((idx, -np.asarray(att, np.float64), -np.asarray(fused, np.float64)))


def slot_topk(row, adds, starts, eos, scale, k):
    """The definition: (tok int32 (k,), fused float32 (k,)) of one slot from the full row."""
    row = np.asarray(row, F32)
    fused = fuse(row, scale, term_row(adds, starts, eos))
    keep = _order(fused, row, np.arange(len(row)))[:k]
    return keep.astype(np.int32), fused[keep]


def class_tables(row, starts, eos, k):
    """idx int32 (2, k), val float32 (2, k) - class 0: not eos, no word start; class 1: word start, not eos; each by (att descending,
    index ascending), padded with -1 / -inf - and the eos entry's value."""
    row = np.asarray(row, F32)
    idx, val = np.full((2, k), -1, np.int32), np.full((2, k), -np.inf, F32)
    for cls in (0, 1):
        members = np.flatnonzero((np.arange(len(row)) != eos) & ((np.asarray(starts) != 0) == bool(cls)))
        best = members[np.argsort(-row[members].astype(np.float64), kind="stable")[:k]]
        idx[cls, :len(best)], val[cls, :len(best)] = best, row[best]
    return idx, val, F32(row[eos])


def slot_topk_from_tables(idx, val, eos_val, adds, eos, scale, k):
    """slot_topk from the class tables: the at most 2k + 1 candidates they hold, fused and ordered by the same rule."""
    tok = np.concatenate([idx[0][idx[0] >= 0], idx[1][idx[1] >= 0], [eos]]).astype(np.int64)
    att = np.concatenate([val[0][idx[0] >= 0], val[1][idx[1] >= 0], [eos_val]]).astype(F32)
    term = np.concatenate([np.zeros((idx[0] >= 0).sum(), F32), np.full((idx[1] >= 0).sum(), F32(adds[0]), F32), [F32(adds[1])]]).astype(F32)
    fused = fuse(att, scale, term)
    keep = _order(fused, att, tok)[:k]
    return tok[keep].astype(np.int32), fused[keep]


def finish(att_out, ylen, ymax, model, vocab, eos, beam_width, lm_scale, length_penalty, sos=1, pad=0, zero_past_len=False, tables=False,
           trace=None):
    """att_out (B, U >= ymax, V) float32 log-probabilities, ylen (B,), ``model`` a ctc_ngram_model.WordModel, ``lm_scale`` =
    float32(lm_weight * ln 10).  Returns per utterance beam_width dicts (hyp, score), best first, as nat_lm_model.fused_finish does.
    ``tables``: candidates from the class tables instead of the full rows.  ``trace``: a list that receives (b, step, slot, adds)."""
    att_out = np.asarray(att_out, F32)
    B, _, V = att_out.shape
    bw = beam_width
    starts = model_of.starts_of(vocab)
    assert len(starts) == V
    last = np.minimum(np.asarray(ylen), ymax - 1)
    st = init_state(B, bw, ymax + 1, sos, pad)
    for step in range(ymax):
        idx = np.zeros((B * bw, bw), np.int32)
        val = np.zeros((B * bw, bw), F32)
        for b in range(B):
            if step > last[b]:
                continue
            row = np.zeros(V, F32) if zero_past_len and step >= ylen[b] else att_out[b, step]
            tab = class_tables(row, starts, eos, bw) if tables else None
            for s in range(b * bw, b * bw + (1 if step == 0 else bw)):
                adds = model_of.adds(model, vocab, st["tok"][s, 1: step + 1].tolist(), eos)
                if trace is not None:
                    trace.append((b, step, s - b * bw, adds))
                idx[s], val[s] = slot_topk_from_tables(*tab, adds, eos, lm_scale, bw) if tables else slot_topk(row, adds, starts, eos, lm_scale, bw)
        st = beam_step(st, idx, val, last, step, bw, pad, length_penalty)
    return [[{"hyp": st["tok"][b * bw + j, : last[b] + 2].tolist(), "score": float(st["score"][b * bw + j])} for j in range(bw)]
            for b in range(B)]
