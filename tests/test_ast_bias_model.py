"""The numpy model of the AST beam search's phrase biasing (tests/ast_bias_model.py): against brute force - the float64 automaton of
tests/ctc_bias_model.py stepped label by label, an implementation of its own - on the nine phrase sets; the identity that the terms
along a hypothesis plus its eos term are the banked score_lm of the CTC search's semantics; the chain of three failure links; and
the case list's power to catch deliberate mistakes.  No GPU, no library."""
import itertools

import numpy as np
import pytest

import ast_bias_cases as cases
import ast_bias_model as model
import ctc_bias_model as ctc_model


def alphabet(phrases, extra=2):
    used = sorted({c for p in phrases for c in p})
    return used[:6] + [cases.IX["▁zz"], cases.IX["cb"]][:extra]


@pytest.mark.parametrize("name", cases.NINE)
def test_node_and_term_are_the_automaton_s_on_every_short_sequence(name):
    """All sequences of up to 4 labels over the set's first pieces and two foreign ones, every candidate of that alphabet and eos."""
    phrases = cases.SETS[name][0]
    aut = ctc_model.Automaton(phrases)
    abc = alphabet(phrases)
    for n in range(5):
        for hyp in itertools.product(abc, repeat=n):
            st = ((), 0.0)
            for c in hyp:
                st = aut.step(st, c)
            assert model.node(hyp, phrases) == st[0], hyp
            for c in abc:
                want = np.float32(aut.slm(aut.step(st, c)) - aut.slm(st)) if phrases else np.float32(0.0)  # (dyadic: exact in float64)
                assert model.term(hyp, phrases, cases.EOS, cases.V, c) == want, (hyp, c)
            assert model.term(hyp, phrases, cases.EOS, cases.V, cases.EOS) == np.float32(st[1] - aut.slm(st)), hyp
            assert model.term(hyp, phrases, cases.EOS, cases.V, -1) == 0 and model.term(hyp, phrases, cases.EOS, cases.V, cases.V) == 0


def test_long_rows_are_the_automaton_s():
    """The 32-piece phrase: every prefix of it, its completion, and the break-off at depth 31."""
    phrases = cases.SETS["long"][0]
    aut = ctc_model.Automaton(phrases)
    row = list(cases.LONG) + list(cases.LONG[:31]) + [cases.IX["▁zz"]]
    st = ((), 0.0)
    for i, c in enumerate(row):
        assert model.node(row[:i], phrases) == st[0]
        assert model.term(row[:i], phrases, cases.EOS, cases.V, c) == np.float32(aut.slm(aut.step(st, c)) - aut.slm(st))
        st = aut.step(st, c)
    assert len(model.node(row[:63], phrases)) == 31 and model.term(row[:63], phrases, cases.EOS, cases.V, row[63]) == np.float32(-31 * 0.5)
    assert model.term(row[:31], phrases, cases.EOS, cases.V, row[31]) == np.float32(32 * 0.5 - 31 * 0.5)


def test_a_stay_and_a_breaker():
    phrases = cases.SETS["shared_prefix"][0]
    a, b = cases.ids("▁a b")
    assert model.node([a, -3, b], phrases) == (a, b)  # a negative id leaves the match where it is
    assert model.node([a, cases.V + 7, b], phrases) == ()  # an id no phrase holds breaks it
    assert model.node([a, 2 ** 31 - 1], phrases) == ()


@pytest.mark.parametrize("name", cases.NINE + ["chain"])
def test_terms_plus_the_eos_term_are_the_banked_score(name):
    """Random sequences of 0 to 40 tokens: what the search adds for a finished hypothesis - every token's term given the tokens
    before it, eos last - is the score_lm the CTC search's semantics give the label sequence; exact, the scores being dyadic."""
    phrases = cases.SETS[name][0]
    rng = np.random.RandomState(len(name))
    used = sorted({c for p in phrases for c in p} | {cases.IX["▁zz"]})
    for trial in range(40):
        seq = [int(t) for t in rng.choice(used, rng.randint(0, 41))]
        total = 0.0
        for i, c in enumerate(seq):
            total += float(model.term(seq[:i], phrases, cases.EOS, cases.V, c))
        total += float(model.term(seq, phrases, cases.EOS, cases.V, cases.EOS))
        assert total == ctc_model.rescan(seq, phrases), seq
        # and without the eos term the open match is still held
        assert total - float(model.term(seq, phrases, cases.EOS, cases.V, cases.EOS)) == ctc_model.rescan(seq, phrases, final=False), seq


def test_the_chain_of_three_failure_links():
    phrases = cases.SETS["chain"][0]
    row, c = cases.CHAIN_ROW, cases.CHAIN_NEXT
    assert model.node(row, phrases) == tuple(row)
    assert model.node(row + [c], phrases) == (cases.IX["bc"], c)
    # value of "▁a b c bc" is 4 * 2, of "bc a" 2 * 2
    assert model.term(row, phrases, cases.EOS, cases.V, c) == np.float32(4.0 - 8.0)
    bias = cases.bias_of("chain")
    n, links = model.node_id(bias, tuple(row)), 0
    while n:
        n, links = int(bias.fail[n]), links + 1
    assert links == 4  # three shorter matches, then the root
    assert model.node_of_id(bias, model.node_id(bias, tuple(row))) == tuple(row)


# ---- the case list catches deliberate mistakes ------------------------------------------------------------------------------------
CATCHERS = {"no_eos": "shared_prefix", "no_reset": "shared_prefix", "no_subtract": "interior", "one_fail": "chain"}


@pytest.mark.parametrize("mistake", model.MISTAKES)
def test_a_deliberate_mistake_in_the_model_is_caught(mistake):
    name = CATCHERS[mistake]
    phrases = cases.SETS[name][0]
    rows = cases.rows_of(name)
    idx = cases.all_candidates(len(rows))
    idx[:, 0] = cases.EOS
    want = cases.model_terms(name, rows, idx)
    wrong = np.array([[model.term(r, phrases, cases.EOS, 2 ** 31 - 1, c, mistake=mistake) for c in idx[k]] for k, r in enumerate(rows)], np.float32)
    assert (want.view(np.int32) != wrong.view(np.int32)).any()
