"""The numpy model of the CASS-NAT finish loop with word n-gram fusion (tests/nat_ngram_model.py) held against itself and against what
already stands: its class-table form equals its full-vocabulary form, with lm_scale 0 it is nat_lm_model.fused_finish with a zero LM, and
the terms along a hypothesis that ends in eos sum to the ARPA score of its text.  No GPU."""
import numpy as np
import pytest

import ast_ngram_model as model_of
import nat_ngram_cases as cases
import nat_ngram_model as nn
from ctc_ngram_model import raw_of
from nat_lm_model import fused_finish

F32 = np.float32
V = 40
VOCAB = cases.vocab_of(V)
STARTS = model_of.starts_of(VOCAB)
ADDS = [(0.0, -1.5), (-2.25, -3.0), (-0.7, -0.1), (-8.0, -8.0), (0.0, 0.0)]


def rows():
    rng = np.random.RandomState(2)
    out = {"random": rng.randn(V).astype(F32) * 3}
    out["ties"] = (-rng.randint(0, 4, V) / 4.0).astype(F32)                     # exact att ties inside and across the classes
    out["zero"] = np.zeros(V, F32)
    # two att values of the word class one ulp apart that meet after the add of a term of 8.0 * scale: the att key decides, not the index
    r = (rng.randn(V).astype(F32) - 5).astype(F32)
    hi, lo = cases.IX["▁ba"], cases.IX["▁ab"]                                   # the better value at the HIGHER index
    assert lo < hi
    r[hi] = F32(1.0)
    r[lo] = np.nextafter(F32(1.0), F32(0.0))
    out["collision"] = r
    return out


@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("name", ["random", "ties", "zero", "collision"])
def test_class_tables_give_the_full_vocabulary_candidates(name, k):
    row = rows()[name]
    idx, val, ev = nn.class_tables(row, STARTS, cases.EOS, k)
    if k == 16:  # V = 40: the class of pieces that start no word has fewer members than the beam
        assert (idx[0] < 0).any() and np.isinf(val[0][idx[0] < 0]).all()
    for adds in ADDS + [(8.0, 1.0)]:
        for scale in (0.5, 1.0, float(F32(0.3 * np.log(10.0)))):
            a, b = nn.slot_topk(row, adds, STARTS, cases.EOS, scale, k)
            c, d = nn.slot_topk_from_tables(idx, val, ev, adds, cases.EOS, scale, k)
            assert a.tolist() == c.tolist(), (name, adds, scale)
            assert b.view(np.int32).tolist() == d.view(np.int32).tolist()


def test_the_collision_case_is_one():
    """fl32(1 + 8) == fl32((1 - ulp) + 8): the (fused, index) rule of the TransformerLM finish would take the lower index first, the
    (fused, att, index) rule takes the better att first - the one case in which the two differ."""
    row = rows()["collision"]
    hi, lo = cases.IX["▁ba"], cases.IX["▁ab"]
    adds = (8.0, 0.0)
    fused = nn.fuse(row, 1.0, nn.term_row(adds, STARTS, cases.EOS))
    assert fused[hi] == fused[lo] and row[hi] > row[lo]
    tok, _ = nn.slot_topk(row, adds, STARTS, cases.EOS, 1.0, 2)
    assert tok.tolist() == [hi, lo]
    assert np.argsort(-fused, kind="stable")[:2].tolist() == [lo, hi]


@pytest.mark.parametrize("lp", [0.1, None])
def test_scale_zero_is_the_lm_finish_with_a_zero_lm(lp):
    _, model = cases.lm_for(3, V)
    att = cases.rows_of(3, 6, V, seed=1)
    ylen = cases.lens_of(3, 6)
    for zero_past_len in (False, True):
        got = nn.finish(att, ylen, 6, model, VOCAB, cases.EOS, 4, 0.0, lp, cases.SOS, cases.PAD, zero_past_len)
        want = fused_finish(att, ylen, 6, lambda ys, mask: np.zeros((len(ys), V), F32), 4, 0.0, lp, cases.SOS, cases.PAD, zero_past_len)
        cases.same_beams(got, want)
    tab = nn.finish(att, ylen, 6, model, VOCAB, cases.EOS, 4, 0.5, lp, cases.SOS, cases.PAD, tables=True)
    cases.same_beams(tab, nn.finish(att, ylen, 6, model, VOCAB, cases.EOS, 4, 0.5, lp, cases.SOS, cases.PAD))


@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_terms_along_a_path_sum_to_the_sentence_score(order):
    """For a hypothesis with one eos, at its end, the terms of its tokens - each under the adds of the tokens before it - sum to
    NgramLM.score of its text."""
    lm, model = cases.lm_for(order, V)
    rng = np.random.RandomState(order)
    pieces = [i for i in range(V) if i != cases.EOS]
    for _ in range(20):
        seq = [int(t) for t in rng.choice(pieces, rng.randint(0, 12))] + [cases.EOS]
        total = 0.0
        for i, c in enumerate(seq):
            total += float(model_of.term(model_of.adds(model, VOCAB, seq[:i], cases.EOS), STARTS, cases.EOS, c))
        want = lm.score(raw_of(seq, VOCAB, drop_id=cases.EOS))
        assert abs(total - want) <= 1e-5 * max(1.0, abs(want)), (seq, total, want)
