"""Inputs shared by the tests of the AST beam search with contextual phrase biasing: the phrase sets (the nine of ctc_bias_cases and
one with a failure chain of three links), token rows that walk them, candidate lists, the host twins as functions with sentinels
behind every output, and the model's answers for a batch of rows."""
import ctypes as C
import functools

import numpy as np

import ast_bias_model as model
import ctc_bias_cases as ctc_cases
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.models.bias import BiasList
from cassnat_asr_public_amd.models.ngram import _ptr
from ctc_bias_cases import IX, LONG, V, VOCAB, ids  # noqa: F401  (re-exported)

EOS, SOS, BLANK = IX["eos"], IX["sos"], IX["blank"]
NEW = ["cn_ast_attach_bias", "cn_op_ast_bias_nodes", "cn_ast_bias_nodes_host", "cn_op_ast_bias_terms", "cn_ast_bias_terms_host",
       "cn_op_logsoftmax_bias_topk", "cn_ast_step_bias"]
SENT_I, SENT_F = -77, -7.5

# "chain": behind "▁a b c bc" the open match shortens three times before "a" finds an edge: ▁a b c bc -> b c bc -> c bc -> bc (+ a)
SETS = dict(ctc_cases.SETS)
SETS["chain"] = ({ids("▁a b c bc cb"): 2.0, ids("b c bc ▁zz"): 0.5, ids("c bc ▁b"): 3.0, ids("bc a ▁c"): 2.0, ids("▁c a b"): 0.5}, 32)
CHAIN_ROW, CHAIN_NEXT = list(ids("▁a b c bc")), IX["a"]
NINE = [n for n in ctc_cases.SETS]
assert len(NINE) == 9


@functools.lru_cache(maxsize=None)
def bias_of(name):
    phrases, bits = SETS[name]
    return BiasList.from_phrases(phrases, hash_bits=bits)


def rows_of(name, ld=41, n_random=30, seed=0):
    """Token rows (lists, at most ld long) that walk set ``name``: the empty row, the phrases whole / cut short / with the last piece
    swapped, two of them glued, each behind a foreign prefix, ids outside the vocabulary, a row of full length, and random rows over
    the pieces the set uses."""
    phrases = SETS[name][0]
    rng = np.random.RandomState(seed + 17 * len(name))
    plants = ctc_cases.plants(phrases)
    rows = [[]] + [list(p)[:ld] for p in plants]
    rows += [(list(a) + list(b))[:ld] for a, b in zip(plants, plants[1:] + plants[:1])]
    rows += [([IX["▁zz"], IX["cb"]] + list(p))[:ld] for p in plants[:4]]
    rows += [[-1], [V + 5, -(2 ** 31), 2 ** 31 - 1], [EOS], [SOS, BLANK]]
    if plants:
        p = list(plants[0])
        rows += [p[:1] + [-3] + p[1:], p[:1] + [V] + p[1:], p[:1] + [1000] + p[1:]]  # a stay inside a match; a breaker inside it
    used = sorted({c for p in phrases for c in p} | {IX["▁zz"], IX["a"]})
    rows.append([int(t) for t in rng.choice(used, ld)])
    for _ in range(n_random):
        rows.append([int(t) for t in rng.choice(used, rng.randint(0, ld + 1))])
    if name == "chain":
        rows.append(list(CHAIN_ROW))
    assert all(len(r) <= ld for r in rows) and any(len(r) == ld for r in rows)
    return rows


def pack(rows, ld, fill=EOS + 1000):
    """(tok (n, ld) int32 with garbage behind every row's length, len (n,) int32)."""
    tok = np.full((len(rows), ld), fill, np.int32)
    for r, row in enumerate(rows):
        tok[r, :len(row)] = row
    return tok, np.array([len(r) for r in rows], np.int32)


def candidates(n, K, rng):
    """idx (n, K) int32: ids of the vocabulary, eos in most rows, now and then an id outside it."""
    idx = rng.randint(0, V, (n, K)).astype(np.int32)
    idx[rng.rand(n, K) < 0.05] = -1
    idx[rng.rand(n, K) < 0.03] = V + 3
    col = rng.randint(0, K)
    idx[np.arange(n) % 4 != 3, col] = EOS
    if K > 1:
        idx[0, (col + 1) % K] = -1
    return idx


def all_candidates(n):
    """Every id of the vocabulary, one below and two above it, for n rows."""
    return np.tile(np.arange(-1, V + 2, dtype=np.int32), (n, 1))


def host_nodes(bias, tok, lens, pad=8, flavour=None):
    n, ld = tok.shape
    out = np.full(n + pad, SENT_I, np.int32)
    L = hip.lib(flavour)
    rc = L.cn_ast_bias_nodes_host(C.byref(bias.desc()), _ptr(tok), ld, _ptr(lens), n, _ptr(out))
    assert rc == 0, L.cn_last_error()
    assert (out[n:] == SENT_I).all()
    return out[:n].copy()


def host_terms(bias, nodes, idx, eos=EOS, pad=8, flavour=None):
    n, K = idx.shape
    nodes = np.ascontiguousarray(nodes, np.int32)
    out = np.full(n * K + pad, SENT_F, np.float32)
    L = hip.lib(flavour)
    rc = L.cn_ast_bias_terms_host(C.byref(bias.desc()), _ptr(nodes), eos, _ptr(np.ascontiguousarray(idx)), n, K, _ptr(out))
    assert rc == 0, L.cn_last_error()
    assert (out[n * K:] == SENT_F).all()
    return out[:n * K].reshape(n, K).copy()


def model_nodes(name, rows):
    """The model's open matches of the rows as node ids of the set's BiasList."""
    bias, phrases = bias_of(name), SETS[name][0]
    return np.array([model.node_id(bias, model.node(r, phrases)) for r in rows], np.int32)


def model_terms(name, rows, idx, eos=EOS, V_=2 ** 31 - 1):
    """The model's terms (n, K) float32 of the candidates idx for the rows (the ids are not bounded above, as the terms entry's)."""
    phrases = SETS[name][0]
    return np.array([model.terms(r, phrases, eos, V_, idx[k]) for k, r in enumerate(rows)], np.float32).reshape(len(rows), -1)


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape
    bad = np.argwhere(a.view(np.int32) != b.view(np.int32))
    assert bad.size == 0, (bad[:5].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])
