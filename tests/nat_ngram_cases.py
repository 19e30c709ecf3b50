"""Inputs shared by the tests of the CASS-NAT finish loop with word n-gram fusion: vocabularies of any size over the n-gram tests' pieces,
their models, log-probability rows, the host entry as a function and the comparison."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np

from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.models.ngram import NgramLM, _ptr
from ctc_ngram_cases import SPELL, IX, WORDS, _dir, collision_case, lm_of
from ctc_ngram_model import WordModel, planted
from ngram_model import random_arpa
from test_gpu_ngram import PIECES

NEW = ["cn_nat_attach_ngram", "cn_nat_ngram_finish", "cn_op_nat_class_topk", "cn_op_nat_ngram_finish", "cn_nat_ngram_finish_host"]
EOS, SOS, PAD = IX["eos"], IX["sos"], IX["blank"]
SENT_I, SENT_F = -77, -7.5


@functools.lru_cache(maxsize=None)
def vocab_of(V):
    """The n-gram tests' pieces, then fillers up to V pieces: continuations "x<i>" and word starts "▁y<i>" in turn (words no model holds).
    At V = 40 the class of pieces that start no word has 14 members: fewer than a beam of 16."""
    assert V >= len(PIECES)
    pieces = PIECES + [("x%d" if i % 2 == 0 else "▁y%d") % i for i in range(V - len(PIECES))]
    return SimpleNamespace(index2word=dict(enumerate(pieces)), word2index={p: i for i, p in enumerate(pieces)}, n_words=V)


@functools.lru_cache(maxsize=None)
def lm_for(order, V, hash_bits=64):
    """(NgramLM over vocab_of(V), WordModel) of ctc_ngram_cases.lm_of's dyadic model of this order."""
    base, model = lm_of(order, hash_bits)
    lm = NgramLM.load(base.path, vocab_of(V), hash_bits=hash_bits)
    assert lm.order == order and lm.device_ok and lm.vocab_size == V
    return lm, model


@functools.lru_cache(maxsize=None)
def plain_lm(V, order=3, seed=6):
    """A model whose values are no dyadic fractions: sums round, and two att values may meet after the add."""
    text = random_arpa(WORDS, order, seed=seed)
    path = os.path.join(_dir(), "nat_plain_%d_%d.arpa" % (order, seed))
    with open(path, "w", encoding="utf-8") as f:
        f.write(text)
    return NgramLM.load(path, vocab_of(V)), WordModel(text)


def rows_of(B, U, V, seed=0, peak=3.0, grid=False):
    """att (B, U, V) float32: random log-softmax rows with planted spellings of words (beams close words in mid-search), or, with
    ``grid``, values on a grid of quarters (exact ties in att and, with a dyadic model and lm_scale 0.5, in the fused values)."""
    rng = np.random.RandomState(100 * U + V + seed)
    if grid:
        return (-rng.randint(0, 12, (B, U, V)) / 4.0).astype(np.float32)
    x = planted(rng, B, U, V, SPELL, peak=peak)
    x[:, :, EOS] += np.float32(1.5)  # eos is a candidate that matters
    return np.ascontiguousarray(x, np.float32)


def lens_of(B, U):
    """ylen per utterance: B = 3 gives one at ylen 0, one cut short, one that consumes every row (ylen >= U: last = U - 1)."""
    return np.array([0, max(0, U // 2), U + 2][:B] + [U] * max(0, B - 3), np.int32)


def run_host(lm, att, ylen, ymax, bw, lm_scale, lp=0.25, use_lp=1, zlen=None, L=None, eos=EOS):
    B, U, V = att.shape
    L = ymax + 1 if L is None else L
    pad = 8
    hyp = np.full(B * bw * L + pad, SENT_I, np.int32)
    hlen = np.full(B * bw + pad, SENT_I, np.int32)
    sc = np.full(B * bw + pad, SENT_F)
    rc = hip.lib().cn_nat_ngram_finish_host(C.byref(lm.desc()), float(np.float32(lm_scale)), _ptr(att), _ptr(ylen), _ptr(zlen) if zlen is not None else None,
                                            B, U, V, ymax, bw, eos, SOS, PAD, use_lp, float(lp), _ptr(hyp), L, _ptr(hlen), _ptr(sc))
    assert rc == 0, hip.lib().cn_last_error()
    assert (hyp[B * bw * L:] == SENT_I).all() and (hlen[B * bw:] == SENT_I).all() and (sc[B * bw:] == SENT_F).all()
    return beams_of(hyp[:B * bw * L].reshape(B, bw, L), hlen[:B * bw].reshape(B, bw), sc[:B * bw].reshape(B, bw))


def beams_of(hyp, hlen, sc, pad=PAD):
    """The entry's arrays as the model's list of lists of dicts; behind a hypothesis its row holds padding."""
    out = []
    for b in range(hyp.shape[0]):
        out.append([{"hyp": hyp[b, j, :hlen[b, j]].tolist(), "score": float(sc[b, j])} for j in range(hyp.shape[1])])
        assert all((hyp[b, j, hlen[b, j]:] == pad).all() for j in range(hyp.shape[1]))
    return out


def same_beams(got, want):
    """Hypotheses, order and float64 scores exact."""
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert [e["hyp"] for e in g] == [e["hyp"] for e in w], b
        assert [e["score"] for e in g] == [e["score"] for e in w], (b, [e["score"] for e in g], [e["score"] for e in w])


def collision_lm(V):
    case = collision_case()
    return lm_for(1, V, case.hash_bits), case


def spelled_rows(words, V, B=3, seed=4, peak=6.0):
    """att (B, U, V) whose best path spells ``words`` (over the letters a, b, c, or "zz" and letters), one piece per row, and ylen."""
    spell = [[IX["▁zz"]] + [IX[c] for c in w[2:]] if w.startswith("zz") else [IX["▁" + w[0]]] + [IX[c] for c in w[1:]] for w in words]
    path = [t for s in spell for t in s] + [IX["▁a"]]
    rng = np.random.RandomState(seed)
    x = rng.randn(B, len(path), V).astype(np.float32)
    for t, piece in enumerate(path):
        x[:, t, piece] += peak
    m = x.max(-1, keepdims=True)
    att = (x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))).astype(np.float32)
    return att, np.array([len(path)] * (B - 1) + [len(path) // 2], np.int32)
