"""float64 restatement of the CTC prefix beam search that merges candidates by prefix (csrc/ctc_merge_search.h; the semantics are in
include/cassnat_hip_ctc_merge.h).  Nothing here comes from the code under test: the schedule is ctc_lm_model.schedule, the candidate
arithmetic and their order are the reference's (per kept hypothesis a stay candidate, then one candidate per pruned non-blank label in
list order; numpy's logaddexp; stable descending sort by (score_ctc + score_lm) + lp * len), sequences are Python tuples.

Between forming a frame's candidates and sorting them: a label that occurred earlier in the frame's list makes no candidate, and an
extension whose tuple equals a kept hypothesis' tuple is folded into that hypothesis' stay candidate (p_nblk' = logaddexp(stay, ext),
p_blk unchanged, score_ctc' = logaddexp(p_blk, p_nblk'), state and score_lm the stay's) and leaves the list.

``scorer``: None (score_lm 0), ``BiasScorer`` or ``NgramScorer`` - the existing models' automaton and word scores.  ``merge=False`` is
the unmerged search of those models.  ``brute_force`` sums all alignments.  ``mistake=NAME`` builds one deliberate mistake in
(tests/test_ctc_merge_model.py shows that the case list catches each): "fold_pb", "keep_ext", "len_last", "stale_tot", "links".
"""
import itertools

import numpy as np

import ctc_bias_model
import ctc_ngram_model
from ctc_lm_model import LOGONE, LOGZERO, schedule

MISTAKES = ("fold_pb", "keep_ext", "len_last", "stale_tot", "links")


class NoScorer(object):
    def init(self):
        return None

    def step(self, state, hyp, c):
        return None

    def slm(self, state):
        return 0.0

    def final(self, state, hyp):
        return 0.0


class BiasScorer(NoScorer):
    """ctc_bias_model's automaton: state (node, banked)."""

    def __init__(self, phrases):
        self.aut = ctc_bias_model.Automaton(phrases)

    def init(self):
        return ((), 0.0)

    def step(self, state, hyp, c):
        return self.aut.step(state, c)

    def slm(self, state):
        return self.aut.slm(state)

    def final(self, state, hyp):
        return state[1]


class NgramScorer(NoScorer):
    """ctc_ngram_model's word scores: state (score_lm, the text of the labels)."""

    def __init__(self, model, vocab, lm_scale):
        self.model, self.vocab, self.lm_scale = model, vocab, lm_scale

    def init(self):
        return (0.0, "")

    def step(self, state, hyp, c):
        closed, _ = ctc_ngram_model.closed_and_open(state[1])
        raw = ctc_ngram_model.raw_of(list(hyp) + [c], self.vocab)
        closed2, _ = ctc_ngram_model.closed_and_open(raw)
        return (ctc_ngram_model.lm_add(self.model, closed, closed2[len(closed):], self.lm_scale, state[0]), raw)

    def slm(self, state):
        return state[0]

    def final(self, state, hyp):
        closed, opened = ctc_ngram_model.closed_and_open(state[1])
        return ctc_ngram_model.lm_add(self.model, closed, ([opened] if opened is not None else []) + ["</s>"], self.lm_scale, state[0])


def frame_labels(top_row, blank, V, merge):
    """The labels of a frame's pruned list that make candidates, in list order."""
    out = []
    for c in top_row:
        c = int(c)
        if c == blank or c < 0 or c >= V or (merge and c in out):
            continue
        out.append(c)
    return out


def search(ctc_out, top, src_size, W, lp, scorer=None, blank=0, merge=True, mistake=None, stats=None):
    """ctc_out (B, T', V) float32, top (B, T', P) pruned labels in list order, src_size (B,) ints.  Returns per utterance the
    best-first list of {'hyp', 'p_blk', 'p_nblk', 'score_ctc', 'score_lm'}.  ``stats`` (a dict): counts the folds and, among them,
    the folds into a hypothesis that was NOT made by extending the extension's parent (a prefix dropped and made again)."""
    assert mistake is None or mistake in MISTAKES
    ctc_out = np.asarray(ctc_out, np.float32)
    V = ctc_out.shape[2]
    sc = scorer or NoScorer()
    out = []
    uid = itertools.count(1)
    for b, frames in enumerate(schedule(ctc_out, src_size, blank)):
        beams = [dict(pb=LOGONE, pnb=LOGZERO, sctc=0.0, st=sc.init(), hyp=(), uid=0, pfx=-1)]
        for t in frames:
            row = ctc_out[b, t]
            cands, stays = [], []
            for h in beams:
                p_b, p_nb, n = h["pb"], h["pnb"], len(h["hyp"])
                last = h["hyp"][-1] if n else -1
                new_p_nb = p_nb + float(row[last]) if n > 0 else LOGZERO
                p_temp = float(row[blank])
                new_p_b = np.logaddexp(p_b + p_temp, p_nb + p_temp)
                stays.append(dict(pb=new_p_b, pnb=new_p_nb, sctc=np.logaddexp(new_p_b, new_p_nb), st=h["st"], hyp=h["hyp"], uid=h["uid"],
                                  pfx=h["pfx"], live=True))
                cands.append(stays[-1])
                for c in frame_labels(top[b, t], blank, V, merge):
                    p_temp = float(row[c])
                    new_p_nb = np.logaddexp(p_b + p_temp, p_nb + p_temp) if c != last else p_b + p_temp
                    cands.append(dict(pb=LOGZERO, pnb=new_p_nb, sctc=np.logaddexp(LOGZERO, new_p_nb), st=sc.step(h["st"], h["hyp"], c),
                                      hyp=h["hyp"] + (c,), uid=None, pfx=h["uid"], live=True))
            if merge:
                for x in cands:
                    if x["uid"] is not None:  # a stay
                        continue
                    if mistake == "len_last":
                        hit = [s for s in stays if len(s["hyp"]) == len(x["hyp"]) and s["hyp"][-1:] == x["hyp"][-1:]]
                    elif mistake == "links":
                        hit = [s for s in stays if s["pfx"] == x["pfx"] and s["hyp"][-1:] == x["hyp"][-1:]]
                    else:
                        hit = [s for s in stays if s["hyp"] == x["hyp"]]
                    if not hit:
                        continue
                    s = hit[0]
                    if stats is not None:
                        stats["folds"] = stats.get("folds", 0) + 1
                        stats["relinked"] = stats.get("relinked", 0) + (s["pfx"] != x["pfx"])
                    s["pnb"] = np.logaddexp(s["pnb"], x["pnb"])
                    if mistake == "fold_pb":
                        s["pb"] = np.logaddexp(s["pb"], x["pnb"])
                    if mistake != "stale_tot":
                        s["sctc"] = np.logaddexp(s["pb"], s["pnb"])
                    x["live"] = mistake == "keep_ext"
                cands = [c for c in cands if c["live"]]
            order = sorted(range(len(cands)), key=lambda i: cands[i]["sctc"] + sc.slm(cands[i]["st"]) + lp * len(cands[i]["hyp"]), reverse=True)[:W]
            beams = [cands[i] for i in order]
            for h in beams:
                if h["uid"] is None:
                    h["uid"] = next(uid)
        for h in beams:
            h["slm"] = sc.final(h["st"], h["hyp"])
        beams = sorted(beams, key=lambda h: h["sctc"] + h["slm"] + lp * len(h["hyp"]), reverse=True)
        out.append([{"hyp": list(h["hyp"]), "p_blk": float(h["pb"]), "p_nblk": float(h["pnb"]), "score_ctc": float(h["sctc"]),
                     "score_lm": float(h["slm"])} for h in beams])
    return out


def collapse(path, blank=0):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return tuple(out)


def brute_force(rows, blank=0):
    """rows (T', V) log-posteriors -> {label sequence: log of the summed probability of all alignments that collapse to it}."""
    rows = np.asarray(rows, np.float64)
    total = {}
    for path in itertools.product(range(rows.shape[1]), repeat=rows.shape[0]):
        p = float(np.exp(sum(rows[t, c] for t, c in enumerate(path))))
        total[collapse(path, blank)] = total.get(collapse(path, blank), 0.0) + p
    return {k: float(np.log(v)) for k, v in total.items()}
