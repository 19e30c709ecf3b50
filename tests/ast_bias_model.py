"""float64 / numpy restatement of what the AST beam search with contextual phrase biasing carries and adds (csrc/ast_bias_search.h;
the semantics are in include/cassnat_hip_ast_bias.h).  Nothing here comes from the code under test and there is no automaton: the
node of a hypothesis and the term of a candidate come from a direct left-to-right rescan of the token list, in the manner of
ctc_bias_model.rescan.

A node is the open match as a tuple of piece ids (() the root): the longest suffix of the labels since the last restart that begins a
listed phrase.  Behind every label the longest suffix of the labels since the last restart that IS a listed phrase banks and restarts.
A negative label is skipped (a stay); a label no phrase holds breaks every match.

``term(hyp, phrases, eos, V, c)``: eos gives the open match up (-value[node], +0.0 at the root); c outside [0, V) adds 0; any other c
adds float32((gain + value[node']) - value[node]) in float64, gain the banked value where the label completes a phrase (node' the
root then), else 0.

``mistake=NAME`` builds one deliberate mistake in (tests/test_ast_bias_model.py shows that the case list catches each): "no_eos" (the
eos term left out), "no_reset" (the gain counted but the match kept open), "no_subtract" (value[node] not taken back), "one_fail"
(the open match shortened once at the most: the failure chain cut to one link).
"""
import numpy as np

from ctc_bias_model import merge, prefix_value

MISTAKES = ("no_eos", "no_reset", "no_subtract", "one_fail")


def value(phrases, prefix):
    """The value of the open match ``prefix`` as a float (0.0 at the root)."""
    return prefix_value(phrases, prefix) if len(prefix) else 0.0


def _open(phrases, seg, one_fail_from=None):
    """The longest suffix of ``seg`` that begins a phrase.  ``one_fail_from`` (the "one_fail" mistake): seg is that open match plus one
    label, and only the whole of it and its longest proper suffix-match plus the label are tried."""
    seg = tuple(seg)
    if one_fail_from is not None:
        n, c = tuple(one_fail_from), seg[-1:]
        tries = [n + c]
        shorter = next((n[k:] for k in range(1, len(n) + 1) if prefix_value(phrases, n[k:]) is not None or k == len(n)), ())
        if n:
            tries.append(tuple(shorter) + c)
        return next((t for t in tries if prefix_value(phrases, t) is not None), ())
    return next((seg[k:] for k in range(len(seg)) if prefix_value(phrases, seg[k:]) is not None), ())


def _done(phrases, seg):
    """The longest suffix of ``seg`` that is a listed phrase, or None."""
    seg = tuple(seg)
    return next((seg[k:] for k in range(len(seg)) if seg[k:] in phrases), None)


def segment(hyp, phrases):
    """The labels since the last restart (negative ones skipped)."""
    phrases = merge(phrases)
    seg = []
    for c in hyp:
        c = int(c)
        if c < 0:
            continue
        seg.append(c)
        if _done(phrases, seg) is not None:
            seg = []
    return seg


def node(hyp, phrases):
    """The open match of the hypothesis ``hyp`` (tokens WITHOUT sos) as a tuple."""
    phrases = merge(phrases)
    return _open(phrases, segment(hyp, phrases))


def term(hyp, phrases, eos, V, c, mistake=None):
    """The float32 term of candidate ``c`` for the hypothesis ``hyp``."""
    return terms(hyp, phrases, eos, V, [c], mistake)[0]


def terms(hyp, phrases, eos, V, cands, mistake=None):
    """The float32 terms of the candidates ``cands`` for the hypothesis ``hyp`` (the hypothesis is scanned once)."""
    assert mistake is None or mistake in MISTAKES
    phrases = merge(phrases)
    if not phrases:
        return np.zeros(len(cands), np.float32)
    seg = segment(hyp, phrases)
    n = _open(phrases, seg)
    vn = value(phrases, n)
    return np.array([_term(phrases, seg, n, vn, eos, V, int(c), mistake) for c in cands], np.float32)


def _term(phrases, seg, n, vn, eos, V, c, mistake):
    if c == eos:
        if mistake == "no_eos":
            return np.float32(0.0)
        return np.float32(-vn) if n else np.float32(0.0)
    if c < 0 or c >= V:
        return np.float32(0.0)
    if mistake == "one_fail":
        n2 = _open(phrases, n + (c,), one_fail_from=n)
        done = _done(phrases, n2)
    else:
        n2 = _open(phrases, seg + [c])
        done = _done(phrases, seg + [c])
    gain = 0.0
    if done is not None:
        gain = value(phrases, done)
        if mistake != "no_reset":
            n2 = ()
    sub = 0.0 if mistake == "no_subtract" else vn
    return np.float32((gain + value(phrases, n2)) - sub)


def nodes(rows, lens, phrases):
    """[node] of the rows (row r: its first lens[r] ids, clamped to the row)."""
    rows = np.asarray(rows)
    return [node(rows[r, :max(0, min(int(lens[r]), rows.shape[1]))].tolist(), phrases) for r in range(rows.shape[0])]


def node_id(bias, n):
    """The id the automaton of models.bias.BiasList gives the open match ``n`` (the test's bridge between the model's tuples and the
    tables' numbers: the trie is walked from the root by its child dicts)."""
    at = 0
    for c in n:
        at = bias.child[at][int(c)]
    return at


def node_of_id(bias, i):
    """The tuple of node ``i`` of a BiasList (by search over the trie)."""
    stack = [(0, ())]
    while stack:
        at, path = stack.pop()
        if at == i:
            return path
        stack += [(m, path + (c,)) for c, m in bias.child[at].items()]
    return ()
