"""tests/ctc_ngram_model.py, the float64 restatement of the CTC prefix beam search with word n-gram fusion, pinned without any code
under test: with lm_scale 0 it is ctc_lm_model's search (itself pinned against the reference's beams) run with all-zero LM rows, and
on dyadic ARPA models every returned score_lm is lm_scale times ArpaModel's score of the hypothesis' text, exactly."""
import numpy as np
import pytest
import torch

import ctc_lm_model
from ctc_ngram_model import WordModel, dyadic_arpa, planted, search
from ngram_model import text_of
from test_gpu_ngram import IX, PIECES, VOCAB, WORDS

V = len(PIECES)
SPELL = [[IX["▁a"], IX["bc"]], [IX["▁ab"], IX["c"]], [IX["▁c"], IX["a"], IX["b"]], [IX["▁zz"], IX["a"]], [IX["▁"]], [IX["▁▁a"], IX["b"]]]


def case(Tp, seed):
    rng = np.random.RandomState(seed)
    logp = planted(rng, 3, Tp, V, SPELL)
    return logp, [Tp, Tp // 2, 0]


@pytest.mark.parametrize("Tp,W,P", [(1, 1, 1), (12, 5, 3), (20, 8, 27), (12, 2, 0)])
def test_with_lm_scale_zero_it_is_the_lm_free_search_of_ctc_lm_model(Tp, W, P):
    logp, sizes = case(Tp, 3 + Tp)
    top = torch.topk(torch.from_numpy(logp), P, dim=-1)[1].numpy() if P else np.zeros((3, Tp, 0), np.int64)
    model = WordModel(dyadic_arpa(WORDS, 3, seed=3))
    got = search(logp, top, sizes, W, 0.3, 0.0, model, VOCAB)
    want = ctc_lm_model.fused_search(logp, sizes, W, P, 0.3, 0.0, lambda ys, mask: np.zeros(V, np.float32))
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert [e["hyp"] for e in g] == [e["hyp"] for e in w]
        for x, y in zip(g, w):
            assert x["score_lm"] == 0.0 and y["score_lm"] == 0.0
            assert (x["score_ctc"], x["p_blk"], x["p_nblk"]) == (y["score_ctc"], y["p_blk"], y["p_nblk"])


@pytest.mark.parametrize("order", [1, 2, 3, 5])
@pytest.mark.parametrize("lm_scale", [0.5, 2.0])
def test_score_lm_is_lm_scale_times_the_text_score_exactly(order, lm_scale):
    model = WordModel(dyadic_arpa(WORDS, order, seed=order, unk=order != 2, keep=0.5 if order < 5 else 0.35))
    logp, sizes = case(24, 40 + order)
    top = np.argsort(-logp, axis=-1, kind="stable")[:, :, :6]
    beams = search(logp, top, sizes, 6, 0.25, lm_scale, model, VOCAB)
    words = 0
    for seqs in beams:
        keys = [e["score_ctc"] + e["score_lm"] + 0.25 * len(e["hyp"]) for e in seqs]
        assert keys == sorted(keys, reverse=True)
        for e in seqs:
            text = text_of(e["hyp"], len(e["hyp"]), VOCAB)
            assert e["score_lm"] == lm_scale * model.score(text)[0], (e, text)
            words += len(text.split())
    # (the words of random beams seldom continue a longer n-gram of the model: the higher orders are reached in tests/test_ngram_host.py)
    assert words > 8 and all(model.hits[k] > 0 for k in range(1, min(order, 2) + 1)), (words, model.hits)


def test_a_large_weight_changes_the_best_hypothesis():
    model = WordModel(dyadic_arpa(WORDS, 3, seed=3))
    logp, sizes = case(24, 11)
    top = np.argsort(-logp, axis=-1, kind="stable")[:, :, :6]
    free = search(logp, top, sizes, 6, 0.0, 0.0, model, VOCAB)
    fused = search(logp, top, sizes, 6, 0.0, 2.0, model, VOCAB)
    assert any(a[0]["hyp"] != b[0]["hyp"] for a, b in zip(free, fused))
