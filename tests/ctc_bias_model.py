"""float64 restatement of the CTC prefix beam search with contextual phrase biasing (csrc/ctc_bias_search.h; the semantics are in
include/cassnat_hip_ctc_bias.h).  Nothing here comes from the code under test: the schedule is ctc_lm_model.schedule, the candidate
arithmetic is the reference's (stay candidate, one candidate per pruned non-blank label, numpy's logaddexp, stable descending sort by
(score_ctc + score_lm) + lp * len), the automaton is built here from dicts (no hash table), and ``rescan`` scores a label sequence
without any automaton at all.

A hypothesis carries (node, banked); a stay candidate has its parent's state; appending label c follows failure links until (node, c)
has an edge or the root is reached, takes the edge (else the root), and where the node's hit is set banks float(bank[node]) and goes
back to the root.  score_lm = banked + float(value[node]); after the last processed frame score_lm = banked and the beam is sorted
once more.

``Automaton(..., mistake=NAME)`` / ``search(..., mistake=NAME)`` build one deliberate mistake in (tests/test_ctc_bias_model.py shows
that the case list catches each): "no_fail", "no_reset", "keep_open", "min_score", "stay_steps".
"""
import numpy as np

from ctc_lm_model import LOGONE, LOGZERO, schedule

MISTAKES = ("no_fail", "no_reset", "keep_open", "min_score", "stay_steps")


def merge(phrases):
    """[(ids, score)] or {ids: score} -> {ids: the largest score}."""
    out = {}
    for ids, s in (phrases.items() if isinstance(phrases, dict) else phrases):
        ids = tuple(int(i) for i in ids)
        out[ids] = max(out.get(ids, -np.inf), float(s))
    return out


def prefix_value(phrases, prefix, pick=max):
    """float32(len) * float32(the largest score of the phrases that begin with ``prefix``) as a float; None when none does."""
    s = [sc for ids, sc in phrases.items() if ids[:len(prefix)] == tuple(prefix)]
    return float(np.float32(len(prefix)) * np.float32(pick(s))) if s else None


class Automaton(object):
    """Nodes are the prefixes of the phrases (tuples; () the root)."""

    def __init__(self, phrases, mistake=None):
        assert mistake is None or mistake in MISTAKES
        self.phrases, self.mistake = merge(phrases), mistake
        self.nodes = {()}
        for ids in self.phrases:
            self.nodes.update(ids[:k] for k in range(1, len(ids) + 1))
        pick = min if mistake == "min_score" else max
        self.value = {n: prefix_value(self.phrases, n, pick) if n else 0.0 for n in self.nodes}
        # fail: the longest proper suffix that is a node; hit: the longest suffix (the node included) that is a phrase
        self.fail = {n: next(n[k:] for k in range(1, len(n) + 1) if n[k:] in self.nodes) for n in self.nodes if n}
        self.hit = {n: next((n[k:] for k in range(len(n)) if n[k:] in self.phrases), None) for n in self.nodes}

    def walk(self, n, c):
        """The node label c leads to from node n, before any bank."""
        while n + (c,) not in self.nodes and n and self.mistake != "no_fail":
            n = self.fail[n]
        return n + (c,) if n + (c,) in self.nodes else ()

    def step(self, state, c):
        n, b = state
        n = self.walk(n, c)
        hit = self.hit[n] if self.mistake != "no_fail" else (n if n in self.phrases else None)
        if hit is not None:
            b = b + self.value[hit]
            if self.mistake != "no_reset":
                n = ()
        return n, b

    def slm(self, state):
        return state[1] + self.value[state[0]]


def rescan(hyp, phrases, final=True):
    """score_lm of a label sequence by a direct left-to-right scan, no automaton: behind every label the longest suffix of the labels
    since the last restart that is a listed phrase banks its value and restarts; the open match (``final`` False) is the longest
    suffix that begins a phrase."""
    phrases = merge(phrases)
    seg, banked = [], 0.0
    for c in hyp:
        seg.append(int(c))
        done = next((tuple(seg[k:]) for k in range(len(seg)) if tuple(seg[k:]) in phrases), None)
        if done is not None:
            # (only a suffix that the open match covers can complete: a phrase is a prefix of itself, so every such suffix does)
            banked += prefix_value(phrases, done)
            seg = []
    if final:
        return banked
    open_ = next((prefix_value(phrases, seg[k:]) for k in range(len(seg)) if prefix_value(phrases, seg[k:]) is not None), 0.0)
    return banked + open_


def events(hyp, phrases):
    """(banks, break-offs) of a label sequence: completed phrases, and labels at which an open match of depth >= 1 got shorter
    without a bank."""
    aut = Automaton(phrases)
    st, banks, breaks = ((), 0.0), 0, 0
    for c in hyp:
        m = aut.walk(st[0], int(c))
        if aut.hit[m] is not None:
            banks += 1
        elif st[0] and len(m) != len(st[0]) + 1:
            breaks += 1
        st = aut.step(st, int(c))
    return banks, breaks


def search(ctc_out, top, src_size, W, lp, phrases, blank=0, mistake=None, gaps=None):
    """ctc_out (B, T', V) float32, top (B, T', P) pruned labels in list order, src_size (B,) ints.  Returns per utterance the
    best-first list of {'hyp', 'p_blk', 'p_nblk', 'score_ctc', 'score_lm'}.  ``gaps`` (a list): gets the difference of the keys on
    both sides of every keep / drop boundary, and of neighbours with different keys in the last sort."""
    ctc_out = np.asarray(ctc_out, np.float32)
    V = ctc_out.shape[2]
    aut = Automaton(phrases, mistake)
    out = []
    for b, frames in enumerate(schedule(ctc_out, src_size, blank)):
        beams = [dict(pb=LOGONE, pnb=LOGZERO, sctc=0.0, st=((), 0.0), hyp=[])]
        for t in frames:
            row = ctc_out[b, t]
            cands = []
            for h in beams:
                p_b, p_nb, n = h["pb"], h["pnb"], len(h["hyp"])
                last = h["hyp"][-1] if n else -1
                new_p_nb = p_nb + float(row[last]) if n > 0 else LOGZERO
                p_temp = float(row[blank])
                new_p_b = np.logaddexp(p_b + p_temp, p_nb + p_temp)
                st = aut.step(h["st"], last) if mistake == "stay_steps" and n else h["st"]
                cands.append(dict(pb=new_p_b, pnb=new_p_nb, sctc=np.logaddexp(new_p_b, new_p_nb), st=st, hyp=h["hyp"]))
                for c in top[b, t]:
                    c = int(c)
                    if c == blank or c < 0 or c >= V:
                        continue
                    p_temp = float(row[c])
                    new_p_nb = np.logaddexp(p_b + p_temp, p_nb + p_temp) if c != last else p_b + p_temp
                    cands.append(dict(pb=LOGZERO, pnb=new_p_nb, sctc=np.logaddexp(LOGZERO, new_p_nb), st=aut.step(h["st"], c), hyp=h["hyp"] + [c]))
            keys = [c["sctc"] + aut.slm(c["st"]) + lp * len(c["hyp"]) for c in cands]
            order = sorted(range(len(cands)), key=lambda i: keys[i], reverse=True)
            if gaps is not None and len(order) > W:
                gaps.append(keys[order[W - 1]] - keys[order[W]])
            beams = [cands[i] for i in order[:W]]
        for h in beams:
            h["slm"] = aut.slm(h["st"]) if mistake == "keep_open" else h["st"][1]
        beams = sorted(beams, key=lambda h: h["sctc"] + h["slm"] + lp * len(h["hyp"]), reverse=True)
        if gaps is not None:
            keys = [h["sctc"] + h["slm"] + lp * len(h["hyp"]) for h in beams]
            gaps.extend(x - y for x, y in zip(keys, keys[1:]) if x != y)
        out.append([{"hyp": list(h["hyp"]), "p_blk": float(h["pb"]), "p_nblk": float(h["pnb"]), "score_ctc": float(h["sctc"]),
                     "score_lm": float(h["slm"])} for h in beams])
    return out
