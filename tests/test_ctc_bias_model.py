"""The float64 model of the CTC prefix beam search with phrase biasing (tests/ctc_bias_model.py) against brute force, the case list's
power to catch deliberate mistakes in it, the planted events, the tie margins of the random cases, and the phrase-list loader
(models/bias.py): its refusals, the duplicate rule, comments, and the invariants of the tables.  No GPU."""
import itertools
import math

import numpy as np
import pytest

import ctc_bias_cases as cases
import ctc_bias_model as model
from cassnat_asr_public_amd.models.bias import BiasList, edge_hash, read_phrases


# ---- the model against brute force ------------------------------------------------------------------------------------------------
TINY_SETS = [
    {},
    {(1,): 2.0},
    {(1, 2): 2.0, (1, 3): 3.0, (1, 2, 4): 0.5},
    {(1, 2, 3, 4): 2.0, (2, 3): 3.0},
    {(1, 1): 2.0, (2, 1, 1): -1.0},
    {(3, 4): -1.0, (4, 3, 4): 3.0, (2,): 0.5},
]


@pytest.mark.parametrize("phrases", TINY_SETS)
def test_every_label_sequence_scores_as_a_rescan(phrases):
    """All sequences of up to 6 labels over 4 pieces: the automaton's banked bonus and open match are the direct scan's."""
    aut = model.Automaton(phrases)
    for n in range(7):
        for hyp in itertools.product(range(1, 5), repeat=n):
            st = ((), 0.0)
            for c in hyp:
                st = aut.step(st, c)
            assert st[1] == model.rescan(hyp, phrases), hyp
            assert aut.slm(st) == model.rescan(hyp, phrases, final=False), hyp


@pytest.mark.parametrize("phrases", TINY_SETS[1:])
@pytest.mark.parametrize("Tp,V", [(1, 3), (2, 5), (3, 5), (4, 5), (4, 4)])
def test_every_kept_hypothesis_scores_as_its_rescan(phrases, Tp, V):
    """T' <= 4, V <= 5, beam 32, full pruning: every kept score_lm is the direct rescan's of its labels.  Candidates are not merged by
    prefix, so V ** T' of them exist: up to two frames nothing is dropped (5 ** 2 <= 32) and all of them are looked at."""
    rng = np.random.RandomState(10 * Tp + V)
    x = rng.randn(2, Tp, V).astype(np.float32)
    logp = (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)
    top = np.tile(np.arange(1, V, dtype=np.int32), (2, Tp, 1))
    got = model.search(logp, top, [Tp, Tp], 32, 0.25, phrases)
    for seqs in got:
        assert 1 <= len(seqs) <= 32
        for e in seqs:
            assert e["score_lm"] == model.rescan(e["hyp"], phrases), e
        keys = [e["score_ctc"] + e["score_lm"] + 0.25 * len(e["hyp"]) for e in seqs]
        assert keys == sorted(keys, reverse=True)
    if V ** Tp <= 32:  # nothing is dropped: every alignment is kept, and every label sequence is among them
        assert all(len(seqs) == V ** Tp for seqs in got)
        assert {tuple(e["hyp"]) for e in got[0]} >= set(itertools.product(range(1, V), repeat=Tp))


# ---- the case list catches deliberate mistakes ------------------------------------------------------------------------------------
CATCHERS = {"no_fail": "interior", "no_reset": "shared_prefix", "keep_open": "shared_prefix", "min_score": "shared_prefix", "stay_steps": "doubled"}


@pytest.mark.parametrize("mistake", model.MISTAKES)
def test_a_deliberate_mistake_in_the_model_is_caught(mistake):
    case = cases.repeat_case() if mistake == "stay_steps" else cases.make_case(40, 5, 3, CATCHERS[mistake])
    want = cases.model_beams(case)
    wrong = model.search(case.logp, case.top, cases.src_sizes(case.ratio, case.logp.shape[1]), case.W, case.lp, cases.SETS[case.name][0],
                         mistake=mistake)
    flat = lambda beams: [(e["hyp"], e["score_lm"]) for seqs in beams for e in seqs]  # noqa: E731
    assert flat(wrong) != flat(want)


# ---- planted events ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in cases.SETS if n not in ("none", "long")])
def test_matches_break_offs_and_banks_occur(name):
    phrases = cases.SETS[name][0]
    banks = breaks = 0
    for beam, pruning in ((5, 3), (32, 8)):
        for seqs in cases.model_beams(cases.make_case(40, beam, pruning, name))[:2]:
            for e in seqs:
                x, y = model.events(e["hyp"], phrases)
                banks, breaks = banks + x, breaks + y
    # (a one-piece phrase banks at once: it has no open match to break off)
    assert banks > 0 and (breaks > 0 or name == "one_piece"), (name, banks, breaks)


def test_the_long_phrase_completes_and_breaks_off_once():
    case = cases.long_case()
    best = cases.model_beams(case)[0][0]
    assert best["hyp"] == case.path and best["score_lm"] == 32 * 0.5
    assert model.events(best["hyp"], cases.SETS["long"][0]) == (1, 1)


def test_an_extending_phrase_is_never_completed():
    phrases = cases.SETS["extends"][0]
    hyp = list(cases.ids("▁c a b"))
    # "▁c a" banks and restarts; its node lies on the way to "▁c a b" and carries that phrase's larger score: 2 * 3, never 3 * 3
    assert model.rescan(hyp, phrases) == 2 * 3.0 and model.rescan(hyp, phrases, final=False) == 2 * 3.0
    aut = model.Automaton(phrases)
    assert aut.value[cases.ids("▁c a")] == 2 * 3.0 and aut.hit[cases.ids("▁c a")] == cases.ids("▁c a")


def test_random_cases_have_no_near_ties():
    """The keys on both sides of every keep / drop boundary (and neighbours of the last sort) differ by more than 1e-9 in the model:
    the 1e-8 agreement of score_ctc cannot reorder anything."""
    for name in cases.SETS:
        for Tp in cases.SHAPES:
            for beam, pruning in cases.BEAMS:
                gaps = []
                cases.model_beams(cases.make_case(Tp, beam, pruning, name), gaps)
                assert all(abs(g) > cases.TIE_GAP for g in gaps), (name, Tp, beam, min(abs(g) for g in gaps))


def test_crafted_rows_tie_exactly():
    case = cases.ties_case()
    ties = 0
    for seqs in cases.model_beams(case):
        keys = [e["score_ctc"] + e["score_lm"] + case.lp * len(e["hyp"]) for e in seqs]
        ties += sum(a == b for a, b in zip(keys, keys[1:]))
    assert ties > 0


# ---- the loader ----------------------------------------------------------------------------------------------------------------------
def write(tmp_path, text, name="bias.txt"):
    p = tmp_path / name
    p.write_text(text, encoding="utf-8")
    return str(p)


def test_loader_reads_scores_comments_and_duplicates(tmp_path):
    text = "# names\n\n▁a bc\n▁c a b\t0.5\n   \n▁a   bc\t2\n▁c a b\t-1\n#▁zz\n▁zz\t3e0\n"
    got = read_phrases(write(tmp_path, text), cases.VOCAB, score=3.0)
    assert got == {cases.ids("▁a bc"): 3.0, cases.ids("▁c a b"): 0.5, cases.ids("▁zz"): 3.0}
    assert read_phrases(write(tmp_path, "▁a bc\n"), cases.VOCAB, score=0.5) == {cases.ids("▁a bc"): 0.5}
    assert BiasList.load(write(tmp_path, "# nothing\n\n"), cases.VOCAB).nodes == 1


@pytest.mark.parametrize("line,what", [("▁a qq", "not in the vocabulary"), ("▁a blank", "cannot be part"), ("sos ▁a", "cannot be part"),
                                       ("▁a eos", "cannot be part"), (" ".join(["a", "b"] * 16 + ["c"]), "33 pieces"), ("▁a\tnan", "not finite"),
                                       ("▁a\tinf", "not finite"), ("▁a\t-inf", "not finite"), ("▁a\tx", "no number"),
                                       ("▁a bc\t2e38", "not finite in float32"), ("▁a\t1e39", "not finite in float32"),
                                       ("▁a b c\t-1.5e38", "not finite in float32")])
def test_loader_refusals_name_the_line(tmp_path, line, what):
    path = write(tmp_path, "▁c\n# c\n" + line + "\n")
    with pytest.raises(ValueError, match=what) as e:
        BiasList.load(path, cases.VOCAB)
    assert "line 3" in str(e.value) and path in str(e.value)


def test_a_32_piece_phrase_loads(tmp_path):
    text = " ".join(cases.PIECES[i] for i in cases.LONG)
    assert BiasList.load(write(tmp_path, text + "\n"), cases.VOCAB).nodes == 33
    with pytest.raises(ValueError, match="finite"):
        BiasList.load(write(tmp_path, "▁a\n"), cases.VOCAB, score=float("nan"))
    # the largest value a 32-piece phrase can carry: 32 * score must stay a finite float32
    assert np.isfinite(BiasList.load(write(tmp_path, text + "\t1e37\n"), cases.VOCAB).value).all()
    with pytest.raises(ValueError, match="line 1.*float32"):
        BiasList.load(write(tmp_path, text + "\t2e37\n"), cases.VOCAB)
    with pytest.raises(ValueError, match="float32"):
        BiasList.from_phrases({(5, 6): 3e38})


@pytest.mark.parametrize("name", list(cases.SETS))
def test_table_invariants(name):
    phrases, bits = cases.SETS[name]
    b, aut = cases.bias_of(name), model.Automaton(phrases)
    assert b.hash_bits == bits and b.slots & (b.slots - 1) == 0 and 4 * (b.edges + 1) <= b.slots < 8 * (b.edges + 1) + 2 and b.nodes == len(aut.nodes)
    # every node is the model's node of the same labels; every edge is found by the probe the device runs
    label = {0: ()}
    for n in range(b.nodes):
        for c, m in b.child[n].items():
            label[m] = label[n] + (c,)
    assert sorted(label.values()) == sorted(aut.nodes)
    starts = set()
    for n in range(b.nodes):
        for c, m in b.child[n].items():
            i = edge_hash(n, c) & ((1 << bits) - 1) & (b.slots - 1)
            starts.add(i)
            for _ in range(b.slots):
                if b.edge_keys[i] == (n << 32) | c:
                    break
                assert b.edge_keys[i] >= 0
                i = (i - 1) & (b.slots - 1)
            assert b.edge_keys[i] == (n << 32) | c and b.edge_child[i] == m
    assert int((b.edge_keys >= 0).sum()) == b.edges == b.nodes - 1
    if name == "probe_wrap":
        assert starts <= {0, 1} and b.edge_keys[b.slots - 1] >= 0  # the runs wrap past slot 0
    ix = {v: k for k, v in label.items()}
    for n in range(b.nodes):
        lab = label[n]
        assert b.depth[n] == len(lab) and b.value[n] == np.float32(aut.value[lab]) and b.value[n].dtype == np.float32
        assert b.fail[n] == (ix[aut.fail[lab]] if lab else 0)
        assert b.hit[n] == (ix[aut.hit[lab]] if aut.hit[lab] is not None else -1)
        assert b.bank[n] == (b.value[b.hit[n]] if b.hit[n] >= 0 else 0.0) and b.reset[n] == (b.hit[n] >= 0)
    assert b.value[0] == 0.0 and b.hit[0] == -1 and not math.isnan(float(b.bank.sum()))
    interior = cases.bias_of("interior")
    lab = {0: ()}
    for n in range(interior.nodes):
        for c, m in interior.child[n].items():
            lab[m] = lab[n] + (c,)
    n = next(k for k, v in lab.items() if v == cases.ids("▁a b c"))
    assert interior.hit[n] != n and lab[interior.hit[n]] == cases.ids("b c") and interior.bank[n] == np.float32(2 * 3.0)
