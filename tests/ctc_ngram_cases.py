"""Inputs shared by tests/test_ctc_ngram_host.py and tests/test_gpu_ctc_ngram_kernel.py: the test vocabulary (test_gpu_ngram's word
and piece lists), dyadic ARPA models of orders 1, 2, 3 and 5 with their float64 models, the cases (log-posteriors, pruned lists, size
ratios and search settings), the host entry as a function, and the comparison."""
import ctypes as C
import functools
import os
import tempfile
from types import SimpleNamespace

import numpy as np

from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.models.ngram import NgramLM, _hash, _ptr
from ctc_ngram_model import WordModel, dyadic_arpa, planted, topk_lists
from test_gpu_ngram import IX, PIECES, VOCAB, WORDS

V = len(PIECES)
ORDERS = (1, 2, 3, 5)
SHAPES = (1, 12, 40)                                   # T'
BEAMS = ((1, 1), (2, 0), (5, 3), (32, 8), (32, 32))    # (ctc_beam, ctc_pruning); pruning is clipped to V - 1 labels
# spellings of multi-piece words of the model, of a word outside it, a bare separator and a doubled one
SPELL = [[IX["▁a"], IX["bc"]], [IX["▁ab"], IX["c"]], [IX["▁a"], IX["b"], IX["c"], IX["bc"]], [IX["▁c"], IX["a"], IX["b"]],
         [IX["▁b"], IX["c"], IX["a"]], [IX["▁c"], IX["bc"]], [IX["▁b"], IX["cb"]], [IX["▁zz"], IX["a"]], [IX["▁"]], [IX["▁▁a"], IX["b"]],
         [IX["▁ba"]], [IX["▁cc"]]]
SENT_I, SENT_F = -77, -7.5


@functools.lru_cache(maxsize=None)
def _dir():
    return tempfile.mkdtemp(prefix="ctc_ngram_")


@functools.lru_cache(maxsize=None)
def lm_of(order, hash_bits=64):
    """(NgramLM, WordModel) of the dyadic model of this order; with hash_bits < 64 the model hears of the collisions of word keys."""
    text = dyadic_arpa(WORDS, order, seed=order, unk=order != 2, keep=0.5 if order < 5 else 0.35)
    path = os.path.join(_dir(), "o%d_%d.arpa" % (order, hash_bits))
    with open(path, "w", encoding="utf-8") as f:
        f.write(text)
    lm = NgramLM.load(path, VOCAB, hash_bits=hash_bits)
    assert lm.order == order and lm.device_ok and lm.unclosed == 0
    alias = None
    if hash_bits < 64:
        mask = (1 << hash_bits) - 1
        model_words = [g[0] for g in WordModel(text).grams if len(g) == 1]
        table = {int(h) & mask: w for w, h in zip(model_words, _hash([w.encode() for w in model_words])[0])}
        memo = {}

        def alias(w):
            if w not in memo:
                memo[w] = w if w in model_words else table.get(int(_hash([w.encode()])[0][0]) & mask, w)
            return memo[w]

    return lm, WordModel(text, alias)


def src_sizes(ratio, Tp):
    """(ratio * T').long() with the product in float32."""
    return [int(np.float32(r) * np.float32(Tp)) for r in ratio]


def make_case(Tp, beam, pruning, order, seed=0, lp=0.25, lm_scale=0.5, B=3):
    """B = 3 utterances: one searched over all its frames, one cut short by its size ratio, one whose every frame is blank."""
    rng = np.random.RandomState(1000 * Tp + 10 * beam + pruning + seed)
    P = min(pruning, V - 1)
    logp = planted(rng, B, Tp, V, SPELL)
    logp[2] = np.log(0.03 / (V - 1))
    logp[2, :, 0] = np.log(0.97)
    ratio = np.array([1.0, 0.55, 1.0], np.float32)[:B]
    return SimpleNamespace(logp=np.ascontiguousarray(logp, np.float32), top=topk_lists(logp, P), ratio=ratio, W=beam, P=P, lp=lp,
                           lm_scale=lm_scale, order=order, hash_bits=64)


def ties_case(order=3):
    """Log-posteriors on a grid of quarters and a dyadic model with lm_scale 0.5: candidates of one parent tie exactly, in score_ctc
    and in the whole key, and the order of the pruned list decides."""
    rng = np.random.RandomState(77)
    B, Tp = 3, 12
    logp = (-rng.randint(1, 9, (B, Tp, V)) / 4.0).astype(np.float32)
    return SimpleNamespace(logp=logp, top=topk_lists(logp, 6), ratio=np.array([1.0, 0.7, 0.3], np.float32), W=5, P=6, lp=0.25, lm_scale=0.5,
                           order=order, hash_bits=64)


def repeat_case(order=2):
    """Every label of the planted path is held for three frames and the pruned list is wide: the last label of a hypothesis is
    among the pruned ones, and a repetition must not append it again."""
    rng = np.random.RandomState(5)
    B, Tp = 3, 18
    path = [IX["▁a"], IX["bc"], IX["▁c"], IX["a"], IX["b"], IX["▁ab"]]
    x = rng.randn(B, Tp, V).astype(np.float32)
    for t in range(Tp):
        x[:, t, path[t // 3]] += 6.0
    m = x.max(-1, keepdims=True)
    logp = (x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))).astype(np.float32)
    return SimpleNamespace(logp=logp, top=topk_lists(logp, 4), ratio=np.ones(B, np.float32), W=4, P=4, lp=0.0, lm_scale=0.5, order=order,
                           hash_bits=64, path=path)


def collision_case():
    """An order-1 model read with the smallest hash_bits at which the file still loads (no two of ITS words or 1-grams share a key)
    and some word the vocabulary can spell shares its masked key with a word of the model; that spelling is planted."""
    import itertools

    spellable = ["".join(s) for n in range(1, 6) for s in itertools.product("abc", repeat=n)] + ["zz", "zza", "zzb", "zzc"]
    for bits in range(6, 20):
        try:
            lm, model = lm_of(1, bits)
        except ValueError:
            continue
        hit = [w for w in spellable if w not in WORDS and model.alias(w) != w]
        if hit:
            break
    else:
        raise AssertionError("no hash_bits gives a collision")
    spell = [[IX["▁zz"]] + [IX[c] for c in w[2:]] if w.startswith("zz") else [IX["▁" + w[0]]] + [IX[c] for c in w[1:]] for w in hit[:4]]
    rng = np.random.RandomState(9)
    logp = planted(rng, 3, 24, V, spell + SPELL[:3], peak=5.0)
    return SimpleNamespace(logp=logp, top=topk_lists(logp, 4), ratio=np.ones(3, np.float32), W=6, P=4, lp=0.1, lm_scale=0.5, order=1,
                           hash_bits=bits, hit=hit)


def outputs(B, W, cap, pad=8):
    """Output arrays with ``pad`` more elements than the entry may write, filled with sentinels."""
    return SimpleNamespace(hyp=np.full(B * W * cap + pad, SENT_I, np.int32), hlen=np.full(B * W + pad, SENT_I, np.int32),
                           sc=np.full(B * W + pad, SENT_F), slm=np.full(B * W + pad, SENT_F), pb=np.full(B * W + pad, SENT_F),
                           pnb=np.full(B * W + pad, SENT_F), nb=np.full(B + pad, SENT_I, np.int32))


def untouched(o, B, W, cap):
    return ((o.hyp[B * W * cap:] == SENT_I).all() and (o.hlen[B * W:] == SENT_I).all() and (o.nb[B:] == SENT_I).all()
            and all((a[B * W:] == SENT_F).all() for a in (o.sc, o.slm, o.pb, o.pnb)))


def beams_of(o, B, W, cap):
    """The entry's arrays as the model's list of lists of dicts."""
    hyp = o.hyp[:B * W * cap].reshape(B, W, cap)
    out = []
    for b in range(B):
        assert 1 <= o.nb[b] <= W
        out.append([{"hyp": hyp[b, j, :o.hlen[b * W + j]].tolist(), "p_blk": float(o.pb[b * W + j]), "p_nblk": float(o.pnb[b * W + j]),
                     "score_ctc": float(o.sc[b * W + j]), "score_lm": float(o.slm[b * W + j])} for j in range(int(o.nb[b]))])
        assert (hyp[b, int(o.nb[b]):] == 0).all() and all((hyp[b, j, o.hlen[b * W + j]:] == 0).all() for j in range(int(o.nb[b])))
    return out


def run_host(case, lm=None, blank=0):
    lm = lm or lm_of(case.order, case.hash_bits)[0]
    B, Tp, _ = case.logp.shape
    cap = Tp + 1
    o = outputs(B, case.W, cap)
    rc = hip.lib().cn_ctc_ngram_beam_host(C.byref(lm.desc()), _ptr(case.logp), _ptr(case.top) if case.P else None, _ptr(case.ratio), B, Tp, V,
                                          case.W, case.P, case.lp, case.lm_scale, blank, _ptr(o.hyp), cap, _ptr(o.hlen), _ptr(o.sc),
                                          _ptr(o.slm), _ptr(o.pb), _ptr(o.pnb), _ptr(o.nb))
    assert rc == 0, hip.lib().cn_last_error()
    assert untouched(o, B, case.W, cap)
    return beams_of(o, B, case.W, cap)


def same_beams(got, want, lm_exact=True, lm_bound=0.0, tol=1e-8):
    """Hypotheses and order exact; score_lm bit for bit (dyadic models) or within lm_bound; score_ctc, p_blk, p_nblk to tol."""
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert [e["hyp"] for e in g] == [e["hyp"] for e in w], b
        for j, (x, y) in enumerate(zip(g, w)):
            if lm_exact:
                assert x["score_lm"] == y["score_lm"], (b, j, x["score_lm"], y["score_lm"])
            else:
                assert abs(x["score_lm"] - y["score_lm"]) <= lm_bound, (b, j, x["score_lm"], y["score_lm"])
            for k in ("score_ctc", "p_blk", "p_nblk"):
                assert abs(x[k] - y[k]) <= tol, (b, j, k, x[k], y[k])
