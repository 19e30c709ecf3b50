"""The weighted edit alignment of include/cassnat_hip_score.h in plain Python integers: the serial recurrence, the tie rule (diagonal,
up, left), the walk.  A helper module of the edit-alignment tests (no test of its own); it shares nothing with the package."""

C, S, D, I = 0, 1, 2, 3
OPS = "CSDI"


def align(ref, hyp, costs=(1, 1, 1)):
    """-> (cost, path): the path in forward order, codes 0 = C, 1 = S, 2 = D, 3 = I."""
    cs, ci, cd = costs
    R, H = len(ref), len(hyp)
    prev = [j * ci for j in range(H + 1)]
    moves = []  # row i - 1: bytearray of H + 1 moves into row i: 0 diagonal, 1 up, 2 left
    for i in range(1, R + 1):
        r = ref[i - 1]
        left = i * cd
        row = [left]
        mv = bytearray(H + 1)
        mv[0] = 1
        for j in range(1, H + 1):
            m = prev[j - 1] + (0 if r == hyp[j - 1] else cs)
            b = 0
            up = prev[j] + cd
            if up < m:
                m, b = up, 1
            lf = left + ci
            if lf < m:
                m, b = lf, 2
            row.append(m)
            mv[j] = b
            left = m
        moves.append(mv)
        prev = row
    cost = prev[H]
    i, j, back = R, H, []
    while i or j:
        b = 2 if i == 0 else moves[i - 1][j]
        if b == 0:
            back.append(C if ref[i - 1] == hyp[j - 1] else S)
            i, j = i - 1, j - 1
        elif b == 1:
            back.append(D)
            i -= 1
        else:
            back.append(I)
            j -= 1
    return cost, back[::-1]


def counts_of(path):
    return [path.count(k) for k in range(4)]


def brute_cost(ref, hyp, costs):
    """The cheapest of ALL alignments, by enumeration (small inputs only)."""
    cs, ci, cd = costs
    best = [None]

    def rec(i, j, c):
        if i == len(ref) and j == len(hyp):
            best[0] = c if best[0] is None else min(best[0], c)
            return
        if i < len(ref) and j < len(hyp):
            rec(i + 1, j + 1, c + (0 if ref[i] == hyp[j] else cs))
        if i < len(ref):
            rec(i + 1, j, c + cd)
        if j < len(hyp):
            rec(i, j + 1, c + ci)

    rec(0, 0, 0)
    return best[0]


def clamp(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def run(case, align_fn=align):
    """What the entry points write for a case of ``edit_cases``: -> (cost [N], counts [N][4], path_len [N], paths [N] lists).  A pair
    one of whose spans leaves its buffer: cost -1, counts 0, path_len 0."""
    cost, counts, plen, paths = [], [], [], []
    memo = {}
    for n in range(case["N"]):
        R = clamp(case["ref_len"][n], 0, case["max_ref"])
        H = clamp(case["hyp_len"][n], 0, case["max_hyp"])
        rb, hb, ob = case["ref_begin"][n], case["hyp_begin"][n], case["ops_begin"][n]
        if rb < 0 or hb < 0 or ob < 0 or rb + R > len(case["ref"]) or hb + H > len(case["hyp"]) or ob + R + H > case["ops_total"]:
            c, p = -1, []
        else:
            key = (rb, R, hb, H)
            if key not in memo:
                memo[key] = align_fn(case["ref"][rb:rb + R], case["hyp"][hb:hb + H], case["costs"])
            c, p = memo[key]
        cost.append(c)
        counts.append(counts_of(p))
        plen.append(len(p))
        paths.append(p)
    return cost, counts, plen, paths
