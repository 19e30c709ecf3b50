"""The named case list of the edit-alignment tests (a helper module, no test of its own): the smallest shapes at which the kernel can
go wrong.  A case is a dict of plain Python values: ``ref`` / ``hyp`` id lists, per pair ``ref_begin`` / ``ref_len`` / ``hyp_begin`` /
``hyp_len`` / ``ops_begin``, ``N``, ``max_ref`` / ``max_hyp``, ``costs`` = (sub, ins, del), ``ops_total``.  Every ops span is followed
by GAP bytes nobody may write.  ``expected`` is the model's answer, computed once per case and shared."""
import functools
import random

import edit_model

COSTS = [(1, 1, 1), (4, 3, 3), (1, 2, 3)]
GAP = 3
SENTINEL = 0xEE
SENT_I = -77


def _case(name, pairs, costs, max_ref=None, max_hyp=None, slack=0):
    """``pairs``: (ref ids, hyp ids) or (ref ids, hyp ids, ref_len, hyp_len) with lengths that may differ from the lists'; the same
    ref list object twice is stored once (a shared reference)."""
    ref, hyp, rb, rl, hb, hl = [], [], [], [], [], []
    seen = {}
    for p in pairs:
        r, h = p[0], p[1]
        if id(r) not in seen:
            seen[id(r)] = len(ref)
            ref += r
        rb.append(seen[id(r)])
        hb.append(len(hyp))
        hyp += h
        rl.append(p[2] if len(p) > 2 else len(r))
        hl.append(p[3] if len(p) > 3 else len(h))
    max_ref = max([0] + rl) + slack if max_ref is None else max_ref
    max_hyp = max([0] + hl) + slack if max_hyp is None else max_hyp
    ob, at = [], 0
    for a, b in zip(rl, hl):
        ob.append(at)
        at += edit_model.clamp(a, 0, max_ref) + edit_model.clamp(b, 0, max_hyp) + GAP
    return {"name": "%s-%d%d%d" % ((name,) + costs), "ref": ref, "hyp": hyp, "ref_begin": rb, "ref_len": rl, "hyp_begin": hb, "hyp_len": hl,
            "ops_begin": ob, "ops_total": at, "N": len(pairs), "max_ref": max_ref, "max_hyp": max_hyp, "costs": costs}


def _ids(rng, n, alphabet):
    return [rng.randrange(alphabet) for _ in range(n)]


def _noisy(rng, ref, alphabet, rate=0.15):
    out = []
    for x in ref:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            out.append(rng.randrange(alphabet))
            continue
        out.append(x)
        if u > 1 - rate / 3:
            out.append(rng.randrange(alphabet))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    rng = random.Random(20260)
    out = []
    for costs in COSTS:
        # R, H in {0, 1, 2}, each against each: all ids equal, and ids that cross
        out.append(_case("tiny-equal", [([5] * R, [5] * H) for R in range(3) for H in range(3)], costs))
        out.append(_case("tiny-cross", [([1, 2][:R], [2, 1][:H]) for R in range(3) for H in range(3)], costs))
        out.append(_case("tiny-slack", [([1, 2][:R], [1, 3][:H]) for R in range(3) for H in range(3)], costs, slack=5))
        # H one below, at and above the workgroup's width: the wave and chunk boundaries of the scan (H + 1 = 64, 65, 66), R likewise
        wide = []
        for R in (5, 63, 64, 65):
            for H in (62, 63, 64, 65, 127, 128, 129):
                r = _ids(rng, R, 4)
                wide.append((r, (_noisy(rng, r, 4) + _ids(rng, H, 4))[:H]))
        out.append(_case("widths", wide, costs))
        # one unit against 300 with the only match at position 0 / at the last position: an insertion run carries across every chunk
        out.append(_case("run-first", [([3], [3] + [4] * 299)], costs))
        out.append(_case("run-last", [([3], [4] * 299 + [3])], costs))
        out.append(_case("run-none", [([3], [4] * 300)], costs))
        out.append(_case("col-first", [([3] + [4] * 299, [3])], costs))
        out.append(_case("col-last", [([4] * 299 + [3], [3])], costs))
        out.append(_case("col-mid", [([4] * 150 + [3] + [4] * 149, [3])], costs))
        same = _ids(rng, 200, 50)
        out.append(_case("equal-200", [(same, list(same))], costs))
        out.append(_case("disjoint", [(_ids(rng, 200, 50), [100 + x for x in _ids(rng, 150, 50)]), ([1] * 40, [2] * 90)], costs))
        # runs of one id: 7 7 7 7 against 7 7 is D D C C
        out.append(_case("runs", [([7] * 4, [7] * 2), ([7] * 2, [7] * 4), ([7] * 10, [7] * 3), ([7, 7, 8, 7, 7], [7, 7]), ([7] * 70, [7] * 66),
                                  ([1, 2, 1, 2, 1], [2, 1, 2]), ([1, 2, 3], [3, 1, 2]), ([1, 2], [3, 4, 1]), ([1, 2, 2, 1], [2, 1, 1, 2, 2])], costs))
        # the 2-bit back-pointers of 1100 x 900 are beyond what the LDS holds
        big = _ids(rng, 1100, 6)
        out.append(_case("big", [(big, _noisy(rng, big, 6, 0.4)[:900])], costs))
        out.append(_case("ids", [([0, -1, 2 ** 31 - 1, -2 ** 31, 0], [-1, 0, 2 ** 31 - 1, 0]), ([-1] * 3, [2 ** 31 - 1] * 3), ([0], [0])], costs))
        one = _ids(rng, 17, 5)
        out.append(_case("n1", [(one, _noisy(rng, one, 5))], costs))
        out.append(_case("n3", [(_ids(rng, 33, 5), _ids(rng, 20, 5)), ([], _ids(rng, 7, 5)), (_ids(rng, 12, 5), [])], costs))
        # 70 ragged pairs, every reference shared by seven of them (hyp lengths whose H + 1 is no multiple of 16 among them)
        refs = [_ids(rng, rng.randrange(0, 41), 8) for _ in range(10)]
        out.append(_case("n70-shared", [(refs[n // 7], _noisy(rng, refs[n // 7], 8, 0.3)) for n in range(70)], costs, slack=1))
        # lengths above max_* and below 0 are clamped
        long_r, long_h = _ids(rng, 50, 4), _ids(rng, 60, 4)
        out.append(_case("clamped", [(long_r, long_h, 50, 60), (long_r, long_h, -3, 60), (long_r, long_h, 50, -1), (long_r, long_h, 2 ** 31 - 1, 2 ** 31 - 1)],
                         costs, max_ref=20, max_hyp=33))
        out.append(_case("max-zero", [([], []), ([1, 2], [3])], costs, max_ref=0, max_hyp=0))
        # a span that leaves its buffer: cost -1, nothing read or written
        bad = _case("span", [([1, 2, 3], [1, 3]), ([1, 2, 3], [1, 3]), ([1, 2, 3], [1, 3]), ([1, 2, 3], [1, 3]), ([1, 2, 3], [1, 3])], costs)
        bad["ref_begin"][1] = -1
        bad["hyp_begin"][2] = len(bad["hyp"]) - 1
        bad["ops_begin"][3] = bad["ops_total"] - 4
        bad["ref_begin"][4] = 2 ** 40
        out.append(bad)
    return out


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def _expected(name):
    return edit_model.run(by_name(name))


def expected(case):
    """-> (cost [N], counts [N][4], path_len [N], ops bytes of ops_total with SENTINEL wherever nothing is written)."""
    cost, counts, plen, paths = _expected(case["name"])
    ops = bytearray([SENTINEL]) * case["ops_total"]
    for n, p in enumerate(paths):
        ops[case["ops_begin"][n]:case["ops_begin"][n] + len(p)] = bytes(p)
    return cost, counts, plen, bytes(ops)


ROWS_BEHIND = 2  # rows behind row N of the per-pair outputs, filled with SENT_I


def run_entry(case, call):
    """Build the arrays of ``case`` (numpy; per-pair outputs with ROWS_BEHIND sentinel rows), hand them to ``call(arrays dict)`` - which
    runs an entry point on them and returns its rc with the outputs as numpy arrays in the same dict - and compare every output byte with
    the model's.  Returns the list of what differed (empty: equal)."""
    import numpy as np

    N = case["N"]
    a = {"ref": np.array(case["ref"] or [0], np.int64).astype(np.int32), "hyp": np.array(case["hyp"] or [0], np.int64).astype(np.int32),
         "ref_total": len(case["ref"]), "hyp_total": len(case["hyp"]), "ops_total": case["ops_total"],
         "ref_begin": np.array(case["ref_begin"], np.int64), "hyp_begin": np.array(case["hyp_begin"], np.int64),
         "ops_begin": np.array(case["ops_begin"], np.int64),
         "ref_len": np.array(case["ref_len"], np.int32), "hyp_len": np.array(case["hyp_len"], np.int32),
         "cost": np.full(N + ROWS_BEHIND, SENT_I, np.int32), "counts": np.full((N + ROWS_BEHIND, 4), SENT_I, np.int32),
         "path_len": np.full(N + ROWS_BEHIND, SENT_I, np.int32), "ops": np.full(case["ops_total"] + GAP, SENTINEL, np.uint8),
         "N": N, "max_ref": case["max_ref"], "max_hyp": case["max_hyp"], "costs": case["costs"]}
    rc = call(a)
    cost, counts, plen, ops = expected(case)
    bad = []
    if rc != 0:
        bad.append("rc %d" % rc)
    if a["cost"].tolist() != cost + [SENT_I] * ROWS_BEHIND:
        bad.append("cost %s != %s" % (a["cost"].tolist()[:8], cost[:8]))
    if a["counts"].tolist() != counts + [[SENT_I] * 4] * ROWS_BEHIND:
        bad.append("counts %s != %s" % (a["counts"].tolist()[:4], counts[:4]))
    if a["path_len"].tolist() != plen + [SENT_I] * ROWS_BEHIND:
        bad.append("path_len %s != %s" % (a["path_len"].tolist()[:8], plen[:8]))
    if a["ops"].tobytes() != ops + bytes([SENTINEL]) * GAP:
        got = a["ops"].tobytes()
        at = next(k for k in range(len(got)) if got[k] != (ops + bytes([SENTINEL]) * GAP)[k])
        bad.append("ops differ first at byte %d" % at)
    return bad
