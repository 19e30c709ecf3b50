"""The numpy model of the CTC token time stamps (tests/ctc_times_model.py) against brute-force enumeration of every path, its status
against the counting criterion, the invariants of its spans over the whole case list, and six deliberate mistakes, each of which at
least one case of the list must catch.  No library, no GPU."""
import itertools
import math

import numpy as np
import pytest

import ctc_times_cases as cases
import ctc_times_model as tm


def same(a, b):
    return (a["status"] == b["status"] and a["start"] == b["start"] and a["end"] == b["end"]
            and np.array_equal(cases.bits(a["conf"]), cases.bits(b["conf"])) and cases.bits(np.float64(a["score"])) == cases.bits(np.float64(b["score"])))


def small_label_rows():
    """Every label sequence of length 0 .. 3 over three symbols, up to renaming: all patterns of repeats."""
    return [[]] + [list(y) for L in (1, 2, 3) for y in itertools.product((1, 2, 3), repeat=L)]


@pytest.mark.parametrize("kind", ["soft", "dyadic"])
def test_model_equals_brute_force_enumeration(kind):
    rows = cases.soft_rows(4, 6, 4, 21) if kind == "soft" else cases.dyadic_rows(4, 6, 4, 22)
    checked = 0
    for b, n in itertools.product(range(4), range(0, 7)):
        for y in small_label_rows():
            got, want = tm.align(rows[b], n, y, cases.BLANK), tm.brute(rows[b], n, y, cases.BLANK)
            assert same(got, want), (kind, b, n, y, got, want)
            checked += got["status"] == 0
    assert checked > 500


def test_brute_force_on_the_spelled_ties_and_minus_inf_rows():
    for name in ("tie_all_zero", "tie_s1_vs_s2", "tie_stay_vs_s1", "tie_end", "no_skip_between_equal"):
        c = cases.case(name)
        for b, w in enumerate(cases.expected(name)):
            L = int(c.label_len[b])
            assert same(w, tm.brute(c.logp[b], int(c.frames[b]), c.labels[b, :L], c.blank)), (name, b)
    # the rules the cases were written for
    assert cases.expected("tie_all_zero")[0]["start"] == [0, 1] and cases.expected("tie_all_zero")[0]["end"] == [1, 5]
    assert cases.expected("tie_all_zero")[1]["start"] == [0] and cases.expected("tie_all_zero")[1]["end"] == [3]
    assert cases.expected("tie_s1_vs_s2")[0]["start"] == [0, 2] and cases.expected("tie_s1_vs_s2")[0]["end"] == [1, 3]
    assert cases.expected("tie_stay_vs_s1")[0]["start"] == [0]
    assert cases.expected("tie_end")[0]["end"] == [3]
    assert cases.expected("no_skip_between_equal")[0]["start"] == [0, 2] and cases.expected("no_skip_between_equal")[0]["score"] == -2.0


def test_status_is_the_counting_criterion_and_spans_are_sound():
    seen = {0: 0, 1: 0, 2: 0}
    for c in cases.cases():
        B, Tp, V = c.logp.shape
        for b, w in enumerate(cases.expected(c.name)):
            n, L = tm.clamp(int(c.frames[b]), 0, Tp), tm.clamp(int(c.label_len[b]), 0, c.labels.shape[1])
            y = c.labels[b, :L].tolist()
            bad = any(v < 0 or v >= V or v == c.blank for v in y)
            assert w["status"] == (2 if bad else (0 if tm.feasible_by_count(y, n) else 1)), (c.name, b)
            seen[w["status"]] += 1
            if w["status"] != 0:
                assert w["start"] == [-1] * L and w["end"] == [-1] * L and not w["conf"].any() and w["score"] == -math.inf
                continue
            if w["score"] == -math.inf:  # (rows holding -inf: every path has probability zero)
                continue
            # spans non-empty, ordered, inside the valid frames; a blank frame between repeated labels
            prev_end = 0
            for u in range(L):
                assert prev_end <= w["start"][u] < w["end"][u] <= n, (c.name, b, u, w)
                if u and y[u] == y[u - 1]:
                    assert w["start"][u] > prev_end, (c.name, b, u)
                prev_end = w["end"][u]
                assert w["conf"][u] == c.logp[b, w["start"][u]:w["end"][u], y[u]].max()
            # the score is the path's own sum, frame by frame
            states = [0] * n
            for u in range(L):
                states[w["start"][u]:w["end"][u]] = [y[u]] * (w["end"][u] - w["start"][u])
            total = float(c.logp[b, 0, states[0] if states[0] else c.blank]) if n else 0.0
            for t in range(1, n):
                total = total + float(c.logp[b, t, states[t] if states[t] else c.blank])
            if c.blank == 0:
                assert total == w["score"], (c.name, b)
    assert seen[0] > 60 and seen[1] >= 8 and seen[2] >= 6, seen


@pytest.mark.parametrize("mistake", tm.MISTAKES)
def test_every_deliberate_mistake_fails_a_case_of_the_list(mistake):
    caught = []
    for c in cases.cases():
        if c.logp.shape[1] > 40 and mistake != "float32":  # (the long rows are needed for the rounding mistake only)
            continue
        wrong = tm.align_batch(c.logp, c.frames, c.labels, c.label_len, c.blank, mistake)
        if not all(same(a, b) for a, b in zip(wrong, cases.expected(c.name))):
            caught.append(c.name)
    assert caught, mistake
