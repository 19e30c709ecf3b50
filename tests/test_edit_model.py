"""The model of the edit alignment (tests/edit_model.py) against brute force, its paths' invariants, and the case list
(tests/edit_cases.py) against deliberate mistakes: every mistake a kernel of this kind is likely to hold must change the answer of at
least one case.  CPU only, no library."""
import itertools

import pytest

import edit_cases
import edit_model

TRIPLES = [(1, 1, 1), (4, 3, 3), (1, 2, 3), (3, 1, 2)]
INF = 1 << 40


def variant(ref, hyp, costs, mistake=None, chunk=64):
    """A copy of the model in the kernel's formulation - a row as a prefix minimum over chunks with a carry, the move from the finished
    cell - into which one ``mistake`` can be put."""
    cs, ci, cd = costs
    if mistake == "swap_ins_del":
        ci, cd = cd, ci
    R, H = len(ref), len(hyp)
    prev = [j * ci for j in range(H + 1)]
    if mistake == "row0_off_by_one":
        prev = [0] + [(j + 1) * ci for j in range(1, H + 1)]
    moves = []
    for i in range(1, R + 1):
        cur, mv = [0] * (H + 1), [0] * (H + 1)
        carry = INF
        for base in range(0, H + 1, chunk):
            if mistake == "carry_dropped" and base > 0:
                carry = INF
            for j in range(base, min(H + 1, base + chunk)):
                if j == 0:
                    t = (i + 1) * cd if mistake == "col0_off_by_one" else i * cd
                    diag = up = None
                else:
                    diag = prev[j - 1] + (0 if ref[i - 1] == hyp[j - 1] else cs)
                    up = prev[j] + cd
                    t = min(diag, up)
                carry = min(carry, t - ci * j)
                d = carry + ci * j
                cur[j] = d
                if j == 0:
                    mv[j] = 1
                    continue
                left = cur[j - 1] + ci
                order = [(diag, 0), (up, 1), (left, 2)]
                if mistake == "up_before_diagonal":
                    order = [(up, 1), (diag, 0), (left, 2)]
                if mistake == "left_before_up":
                    order = [(diag, 0), (left, 2), (up, 1)]
                mv[j] = next((b for v, b in order if v == d), 2)
        moves.append(mv)
        prev = cur
    i, j, back = R, H, []
    for _ in range(R + H):
        if i == 0 and j == 0:
            break
        b = 2 if i == 0 else (1 if j == 0 else moves[i - 1][j])
        if b == 0:
            back.append(edit_model.C if ref[i - 1] == hyp[j - 1] else edit_model.S)
            i, j = i - 1, j - 1
        elif b == 1:
            back.append(edit_model.D)
            i -= 1
        else:
            back.append(edit_model.I)
            j -= 1
    return prev[H], (back if mistake == "path_reversed" else back[::-1])


MISTAKES = ["swap_ins_del", "up_before_diagonal", "left_before_up", "row0_off_by_one", "col0_off_by_one", "carry_dropped", "path_reversed"]


def small_cases():
    return [c for c in edit_cases.cases() if not c["name"].startswith("big")]


def test_model_cost_is_brute_force_minimum():
    # (only equality of ids is read, so a reference whose ids appear in the order 0, 1, 2 stands for all its relabelings)
    def first_use_order(seq):
        return all(x <= max(seq[:k], default=-1) + 1 for k, x in enumerate(seq))

    for alphabet in (2, 3):
        for R in range(5):
            for H in range(5):
                for ref in filter(first_use_order, itertools.product(range(alphabet), repeat=R)):
                    for hyp in itertools.product(range(alphabet), repeat=H):
                        for costs in TRIPLES:
                            cost, path = edit_model.align(list(ref), list(hyp), costs)
                            assert cost == edit_model.brute_cost(ref, hyp, costs), (ref, hyp, costs)


def test_paths_account_for_both_sides_and_the_cost():
    for case in edit_cases.cases():
        cs, ci, cd = case["costs"]
        cost, counts, plen, paths = edit_cases._expected(case["name"])
        for n in range(case["N"]):
            if cost[n] < 0:
                assert counts[n] == [0, 0, 0, 0] and plen[n] == 0
                continue
            R = edit_model.clamp(case["ref_len"][n], 0, case["max_ref"])
            H = edit_model.clamp(case["hyp_len"][n], 0, case["max_hyp"])
            c, s, d, i = counts[n]
            assert c + s + d == R and c + s + i == H and plen[n] == c + s + d + i
            assert cost[n] == s * cs + i * ci + d * cd


def test_four_sevens_against_two():
    assert edit_model.align([7, 7, 7, 7], [7, 7]) == (2, [edit_model.D, edit_model.D, edit_model.C, edit_model.C])


def test_variant_without_mistake_is_the_model():
    for case in small_cases():
        assert edit_model.run(case, lambda r, h, c: variant(r, h, c)) == edit_cases._expected(case["name"]), case["name"]
    for chunk in (1, 2, 3):  # (the prefix-minimum identity at every chunk width)
        for case in small_cases()[:12]:
            assert edit_model.run(case, lambda r, h, c: variant(r, h, c, chunk=chunk)) == edit_cases._expected(case["name"]), case["name"]


@pytest.mark.parametrize("mistake", MISTAKES)
def test_case_list_catches(mistake):
    caught = [case["name"] for case in small_cases()
              if edit_model.run(case, lambda r, h, c: variant(r, h, c, mistake)) != edit_cases._expected(case["name"])]
    assert caught, "no case of the list notices the mistake %r" % mistake
