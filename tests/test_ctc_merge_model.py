"""The float64 model of the merging CTC prefix beam search (tests/ctc_merge_model.py) against a sum over all alignments, its
invariants, and five planted mistakes, each caught by the case list the host and kernel tests share (tests/ctc_merge_cases.py)."""
import functools

import numpy as np
import pytest

import ctc_bias_cases
import ctc_bias_model
import ctc_merge_cases as cases
import ctc_merge_model as model

BRUTE_TOL, BRUTE_FLOOR = 1e-9, -50.0  # float64 sums of a few hundred terms; anything near CS_LOGZERO is skipped


@functools.lru_cache(maxsize=None)
def brute_case(Tp, seed):
    """Blank plus 2 labels, both in every pruned list (in the order of their posteriors), blank posteriors at or below 0.95."""
    rng = np.random.RandomState(100 * Tp + seed)
    x = rng.randn(1, Tp, 3) * (0.5 + seed % 3)
    p = np.exp(x - x.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    over = p[..., 0] > 0.9
    p[over] = np.array([0.9, 0.04, 0.06])
    logp = np.log(p).astype(np.float32)
    assert (np.exp(logp[..., 0]) <= 0.95).all()
    top = np.argsort(-logp[..., 1:], axis=-1, kind="stable").astype(np.int32) + 1
    return logp, top


def brute_errors(Tp, seed, merge):
    logp, top = brute_case(Tp, seed)
    beams = model.search(logp, top, [Tp], 31, 0.0, merge=merge)[0]
    want = model.brute_force(logp[0].astype(np.float64))
    errs = []
    for e in beams:
        if e["score_ctc"] > BRUTE_FLOOR:
            errs.append(abs(e["score_ctc"] - want[tuple(e["hyp"])]))
    return beams, want, errs


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("Tp", [1, 2, 3, 4])
def test_score_ctc_is_the_sum_over_all_alignments(Tp, seed):
    beams, want, errs = brute_errors(Tp, seed, True)
    # a beam as wide as the number of label sequences drops none: every sequence an alignment collapses to is there, once (beside
    # them sequences no alignment of T' frames spells, such as "1 1" in two frames, with scores near CS_LOGZERO)
    hyps = [tuple(e["hyp"]) for e in beams]
    assert len(set(hyps)) == len(hyps) and set(want) <= set(hyps)
    assert {tuple(e["hyp"]) for e in beams if e["score_ctc"] > BRUTE_FLOOR} == {k for k, v in want.items() if v > BRUTE_FLOOR}
    assert errs and max(errs) <= BRUTE_TOL, max(errs)
    for e in beams:
        assert abs(np.logaddexp(e["p_blk"], e["p_nblk"]) - e["score_ctc"]) <= 1e-12


def test_the_unmerged_search_fails_the_brute_force_check():
    """The check shows the feature and not the harness: without merging score_ctc is the score of a bundle of paths."""
    worst = 0.0
    for Tp in (2, 3, 4):
        for seed in range(6):
            beams, want, errs = brute_errors(Tp, seed, False)
            worst = max([worst] + errs)
            if Tp >= 2:
                hyps = [tuple(e["hyp"]) for e in beams]
                assert len(set(hyps)) < len(hyps)  # (and the beam holds duplicates)
    assert worst > 1e-3


ALL_CASES = [("crafted", n) for n in cases.CRAFTED] + [("make", (12, 5, 8)), ("make", (40, 20, 30)), ("make", (12, 32, 32)), ("make", (40, 3, 0)),
                                                       ("make", (12, 1, 3))]


def case_of(kind, arg):
    return cases.crafted(arg) if kind == "crafted" else cases.make_case(*arg)


@pytest.mark.parametrize("policy", cases.POLICIES)
@pytest.mark.parametrize("kind,arg", ALL_CASES)
def test_final_beams_hold_pairwise_different_sequences(kind, arg, policy):
    case = case_of(kind, arg)
    for seqs in cases.model_beams(case, policy):
        hyps = [tuple(e["hyp"]) for e in seqs]
        assert len(set(hyps)) == len(hyps)


def test_the_case_list_has_what_it_says():
    st = {}
    cases.model_beams(cases.relink_case(), "none", stats=st)
    assert st["relinked"] >= 1  # a fold that no slot link joins
    for policy in cases.POLICIES:
        st = {}
        cases.model_beams(cases.crafted("abc40_wide"), policy, stats=st)
        assert st["relinked"] >= 1 and st["folds"] >= 40 * 3  # nearly every frame folds, and more than 256 candidates a frame
        st = {}
        cases.model_beams(cases.runs_case(), policy, stats=st)
        assert st["folds"] >= 10
    assert cases.model_beams(cases.runs_case(), "none")[0][0]["hyp"] == cases.runs_case().labels
    dup = cases.duplicate_case()
    assert any(len(set(row.tolist())) < len(row) for row in dup.top.reshape(-1, dup.P))
    unmerged = cases.model_beams(cases.crafted("abc40"), "none", merge=False)
    assert any(len({tuple(e["hyp"]) for e in seqs}) < len(seqs) for seqs in unmerged)


@pytest.mark.parametrize("policy", cases.POLICIES)
@pytest.mark.parametrize("W,P", [(1, 0), (1, 3), (3, 0)])
def test_nothing_to_fold_is_the_unmerged_search_exactly(W, P, policy):
    for case in (cases.alphabet_case(12, W, P, seed=3), cases.make_case(12, W, P)):
        assert cases.model_beams(case, policy) == cases.model_beams(case, policy, merge=False)


def test_the_unmerged_model_is_the_sibling_models():
    case = cases.make_case(12, 5, 8)
    want = ctc_bias_model.search(case.logp, case.top, cases.src_sizes(case.ratio, 12), case.W, case.lp, ctc_bias_cases.SETS[cases.PHRASES][0])
    assert cases.model_beams(case, "bias", merge=False) == want


@pytest.mark.parametrize("name", ["abc40", "runs", "relink", "duplicate", "abc_lp"])
def test_no_fusion_in_disguise_gives_the_lm_free_beams(name):
    case = cases.crafted(name)
    want = cases.model_beams(case, "none")
    sizes = cases.src_sizes(case.ratio, case.logp.shape[1])
    empty = model.search(case.logp, case.top, sizes, case.W, case.lp, model.BiasScorer({}))
    scale0 = model.search(case.logp, case.top, sizes, case.W, case.lp, model.NgramScorer(cases.scorer_of("ngram").model, cases.VOCAB, 0.0))
    for got in (empty, scale0):
        assert [[e["hyp"] for e in s] for s in got] == [[e["hyp"] for e in s] for s in want]
        for g, w in zip(got, want):
            for x, y in zip(g, w):
                assert x["score_lm"] == 0.0 and all(x[k] == y[k] for k in ("score_ctc", "p_blk", "p_nblk"))


def differs(got, want, tol=1e-6):
    if [[e["hyp"] for e in s] for s in got] != [[e["hyp"] for e in s] for s in want]:
        return True
    return any(abs(x[k] - y[k]) > tol for g, w in zip(got, want) for x, y in zip(g, w) for k in ("score_ctc", "p_blk", "p_nblk"))


@pytest.mark.parametrize("mistake", model.MISTAKES)
def test_planted_mistakes_are_caught(mistake):
    caught = []
    for name in ("abc40", "runs", "relink", "duplicate", "abc_lp"):
        case = cases.crafted(name)
        bad = model.search(case.logp, case.top, cases.src_sizes(case.ratio, case.logp.shape[1]), case.W, case.lp, None, mistake=mistake)
        if differs(bad, cases.model_beams(case, "none")):
            caught.append(name)
    assert caught, mistake
    if mistake == "links":  # (links between slots alone miss the fold into a hypothesis whose prefix was dropped and made again)
        assert "relink" in caught
    if mistake == "len_last":
        assert "runs" in caught or "abc40" in caught
