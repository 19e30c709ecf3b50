"""float64 restatement of the CTC prefix beam search with word n-gram fusion (csrc/ctc_ngram_search.h; the semantics are in
include/cassnat_hip_ctc_ngram.h).  Nothing here comes from the code under test: the schedule is ctc_lm_model.schedule, the candidate arithmetic
is ctc_lm_model.frame_step's (stay candidate, one candidate per pruned non-blank label, numpy's logaddexp, stable descending sort by
(score_ctc + score_lm) + lp * len), the words are the ones ngram_model.text_of finds, the scores are ArpaModel's.

score_lm: a stay candidate has its parent's; a candidate that appends label c adds, for every word that c closes (at most one: a
piece carries separators only in front), float(word score) * lm_scale, the word score being the float32 sum of the ARPA terms in
their order (probability, then back-off weights) given the words closed before it.  After the last frame every kept hypothesis adds
its open word, then </s>, and the beam is sorted once more by the same key.
"""
import re

import numpy as np

from ctc_lm_model import LOGONE, LOGZERO, schedule
from ngram_model import UNK_MISSING, ArpaModel, random_arpa, text_of


class WordModel(ArpaModel):
    """ArpaModel that also gives one word's score after a history.  ``alias`` (word -> word): a test with a small hash_bits tells
    the model which words the library's masked key takes for a word of the model (it asks cn_ngram_hash)."""

    def __init__(self, text, alias=None):
        ArpaModel.__init__(self, text)
        self.alias = alias
        self._memo = {}

    def known(self, w):
        if self.alias is not None:
            w = self.alias(w)
        return w if (w,) in self.grams else "<unk>"

    def word_terms(self, hist, w):
        """ARPA terms of word ``w`` (already mapped by ``known``) after the words ``hist`` (``<s>`` first): ArpaModel.score's loop body."""
        c = min(self.order - 1, len(hist))
        ctx = list(hist[len(hist) - c:])
        k, p = 1, UNK_MISSING
        for kk in range(c + 1, 0, -1):
            g = tuple(ctx[c - (kk - 1):]) + (w,)
            if g in self.grams:
                k, p = kk, self.grams[g][0]
                break
        self.hits[k] += 1
        terms = [p]
        for j in range(k, c + 1):
            g = tuple(ctx[c - j:])
            if g in self.grams and self.grams[g][1] is not None:
                terms.append(self.grams[g][1])
        return terms

    def word_score(self, hist, w):
        """The float32 sum of the terms in their order, as a float."""
        key = (tuple(hist[-(self.order - 1):]) if self.order > 1 else (), w)
        if key not in self._memo:
            s = np.float32(0.0)
            for i, t in enumerate(self.word_terms(hist, w)):
                s = np.float32(t) if i == 0 else np.float32(s + np.float32(t))
            self._memo[key] = float(s)
        return self._memo[key]


def raw_of(hyp, vocab, drop_id=2):
    """text_of's text before the strip: a blank at its end says that no word is open."""
    return "".join(vocab.index2word[int(t)] for t in hyp if int(t) != drop_id).replace("▁", " ")


def closed_and_open(raw):
    words = raw.split()
    if raw and not raw[-1].isspace():
        return words[:-1], words[-1]
    return words, None


def lm_add(model, closed_before, new_words, lm_scale, slm):
    """slm plus float(word score) * lm_scale for each of new_words in turn, after the words closed_before."""
    hist = ["<s>"] + [model.known(w) for w in closed_before]
    for w in new_words:
        w = model.known(w)
        slm = slm + model.word_score(hist, w) * lm_scale
        hist.append(w)
    return slm


def search(ctc_out, top, src_size, W, lp, lm_scale, model, vocab, blank=0):
    """ctc_out (B, T', V) float32, top (B, T', P) pruned labels in list order, src_size (B,) ints.  Returns per utterance the
    best-first list of {'hyp', 'p_blk', 'p_nblk', 'score_ctc', 'score_lm'}."""
    ctc_out = np.asarray(ctc_out, np.float32)
    out = []
    for b, frames in enumerate(schedule(ctc_out, src_size, blank)):
        beams = [dict(pb=LOGONE, pnb=LOGZERO, sctc=0.0, slm=0.0, hyp=[], raw="")]
        for t in frames:
            row = ctc_out[b, t]
            cands = []
            for h in beams:
                p_b, p_nb, n = h["pb"], h["pnb"], len(h["hyp"])
                last = h["hyp"][-1] if n else -1
                closed, opened = closed_and_open(h["raw"])
                new_p_nb = p_nb + float(row[last]) if n > 0 else LOGZERO
                p_temp = float(row[blank])
                new_p_b = np.logaddexp(p_b + p_temp, p_nb + p_temp)
                cands.append(dict(pb=new_p_b, pnb=new_p_nb, sctc=np.logaddexp(new_p_b, new_p_nb), slm=h["slm"], hyp=h["hyp"], raw=h["raw"]))
                for c in top[b, t]:
                    c = int(c)
                    if c == blank:
                        continue
                    p_temp = float(row[c])
                    new_p_nb = np.logaddexp(p_b + p_temp, p_nb + p_temp) if c != last else p_b + p_temp
                    raw = raw_of(h["hyp"] + [c], vocab)
                    closed2, _ = closed_and_open(raw)
                    assert closed2[:len(closed)] == closed and len(closed2) - len(closed) <= 1
                    slm = lm_add(model, closed, closed2[len(closed):], lm_scale, h["slm"])
                    cands.append(dict(pb=LOGZERO, pnb=new_p_nb, sctc=np.logaddexp(LOGZERO, new_p_nb), slm=slm, hyp=h["hyp"] + [c], raw=raw))
            order = sorted(range(len(cands)), key=lambda i: cands[i]["sctc"] + cands[i]["slm"] + lp * len(cands[i]["hyp"]), reverse=True)[:W]
            beams = [cands[i] for i in order]
        for h in beams:
            assert h["raw"].strip() == text_of(h["hyp"], len(h["hyp"]), vocab)
            closed, opened = closed_and_open(h["raw"])
            h["slm"] = lm_add(model, closed, ([opened] if opened is not None else []) + ["</s>"], lm_scale, h["slm"])
        beams = sorted(beams, key=lambda h: h["sctc"] + h["slm"] + lp * len(h["hyp"]), reverse=True)
        out.append([{"hyp": list(h["hyp"]), "p_blk": float(h["pb"]), "p_nblk": float(h["pnb"]), "score_ctc": float(h["sctc"]),
                     "score_lm": float(h["slm"])} for h in beams])
    return out


_NUM = re.compile(r"^-?\d")


def dyadic_arpa(words, order, seed, unk=True, keep=0.5):
    """random_arpa's closed structure with dyadic values: every log-probability and back-off weight a multiple of 1/64 in [-4, 0]
    (<s> stays -99), so that every float32 word score and every float64 product with a power-of-two lm_scale is exact."""
    rng = np.random.RandomState(1000 + seed)
    out = []
    for line in random_arpa(words, order, seed, unk=unk, keep=keep).split("\n"):
        f = line.split("\t")
        if len(f) >= 2 and _NUM.match(f[0]):
            if f[0] != "-99":
                f[0] = "%.6f" % (-rng.randint(1, 257) / 64.0)
            if len(f) == 3:
                f[2] = "%.6f" % (-rng.randint(0, 257) / 64.0)
        out.append("\t".join(f))
    return "\n".join(out)


def planted(rng, B, Tp, V, words_ix, blank=0, peak=3.0, blank_bias=0.0):
    """Random log-softmax rows (B, T', V) float32 with a planted path: per utterance the pieces of some multi-piece words, a few
    frames each with blanks between, lifted by ``peak`` so that beams follow them and close words in mid-search."""
    x = rng.randn(B, Tp, V).astype(np.float32)
    x[:, :, blank] += blank_bias
    for b in range(B):
        t = 0
        while t < Tp:
            for piece in words_ix[rng.randint(len(words_ix))]:
                for _ in range(rng.randint(1, 3)):
                    if t < Tp:
                        x[b, t, piece] += peak
                        t += 1
                if rng.rand() < 0.4 and t < Tp:
                    x[b, t, blank] += peak
                    t += 1
    m = x.max(-1, keepdims=True)
    return (x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))).astype(np.float32)


def topk_lists(ctc_out, P):
    """(B, T', P) labels by falling log-posterior; among equal values the smaller id first."""
    if P == 0:
        return np.zeros(ctc_out.shape[:2] + (0,), np.int32)
    return np.argsort(-ctc_out.astype(np.float64), axis=-1, kind="stable")[:, :, :P].astype(np.int32)
