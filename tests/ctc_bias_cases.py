"""Inputs shared by tests/test_ctc_bias_host.py and tests/test_gpu_ctc_bias_kernel.py: the test vocabulary (test_gpu_ngram's piece
list), the phrase sets with dyadic scores (0.5, 2, 3, -1), the cases (log-posteriors with planted phrases and near-misses, pruned
lists, size ratios and search settings), the float64 model's result per case (computed once), the host entry as a function."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np

import ctc_bias_model as model
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.models.bias import BiasList
from cassnat_asr_public_amd.models.ngram import _ptr
from ctc_ngram_cases import SENT_F, SENT_I, beams_of, outputs, same_beams, src_sizes, untouched  # noqa: F401 (the comparison is the n-gram search's)
from ctc_ngram_model import planted, topk_lists
from test_gpu_ngram import IX, PIECES

V = len(PIECES)
VOCAB = SimpleNamespace(index2word=dict(enumerate(PIECES)), word2index=dict(IX), n_words=V)
SHAPES = (1, 12, 40)                                   # T'
BEAMS = ((1, 1), (2, 0), (5, 3), (32, 8), (32, 32))    # (ctc_beam, ctc_pruning); pruning is clipped to V - 1 labels: 32 * 28 > 256 candidates
TIE_GAP = 1e-9


def ids(text):
    return tuple(IX[p] for p in text.split())


LONG = tuple(IX[p] for p in ("▁a", "b", "c", "bc", "cb", "a", "▁b", "c") * 4)  # 32 pieces, no piece twice in a row
assert len(LONG) == 32
# name -> (phrases {ids: per-piece score}, hash_bits)
SETS = {
    "none": ({}, 32),
    "one_piece": ({ids("▁a"): 2.0}, 32),
    "shared_prefix": ({ids("▁a b c"): 2.0, ids("▁a bc"): 3.0, ids("▁a b cb"): 0.5, ids("▁c a b"): 2.0}, 32),
    "interior": ({ids("▁a b c bc"): 2.0, ids("b c"): 3.0, ids("▁c a b"): 0.5}, 32),        # `hit` of "▁a b c" comes from its failure chain
    "extends": ({ids("▁c a"): 2.0, ids("▁c a b"): 3.0, ids("▁a bc"): 0.5}, 32),            # "▁c a b" is never completed
    "doubled": ({ids("▁a b b c"): 2.0, ids("▁b c c"): 3.0, ids("c c"): 0.5}, 32),           # repetition meets the stay rule
    "long": ({LONG: 0.5, ids("▁c a b"): 2.0}, 32),
    "negative": ({ids("▁a bc"): -1.0, ids("▁c a b"): -1.0, ids("▁ab c"): 2.0}, 32),
    "probe_wrap": ({ids("▁a b c"): 2.0, ids("▁a bc"): 3.0, ids("▁ab c"): 0.5, ids("▁c a b"): 2.0, ids("▁b c a"): 3.0, ids("▁c bc"): 0.5,
                    ids("▁b cb"): 2.0, ids("▁zz a"): -1.0, ids("▁a b c bc"): 2.0, ids("b c"): 0.5}, 1),  # every probe starts at slot 0 or 1
}
# per set: seeds of make_case for which the model's keys at every keep / drop boundary differ by more than TIE_GAP ((T', beam) -> seed)
SEEDS = {}


def plants(phrases):
    """The phrases, each phrase cut short by one piece and each with its last piece swapped: matches, break-offs and banks."""
    out = []
    for p in sorted(phrases):
        p = list(p)
        out += [p, p[:-1] + [IX["cb"] if p[-1] != IX["cb"] else IX["a"]]] + ([p[:-1]] if len(p) > 1 else [])
    return out or [[IX["▁a"], IX["bc"]], [IX["▁c"]]]


@functools.lru_cache(maxsize=None)
def bias_of(name):
    phrases, bits = SETS[name]
    return BiasList.from_phrases(phrases, hash_bits=bits)


@functools.lru_cache(maxsize=None)
def make_case(Tp, beam, pruning, name, lp=0.25, B=3):
    """B = 3 utterances: one searched over all its frames, one cut short by its size ratio, one whose every frame is blank."""
    seed = SEEDS.get((name, Tp, beam), 0)
    rng = np.random.RandomState(1000 * Tp + 10 * beam + pruning + 7919 * seed)
    P = min(pruning, V - 1)
    logp = planted(rng, B, Tp, V, plants(SETS[name][0]), peak=4.0)
    logp[2] = np.log(0.03 / (V - 1))
    logp[2, :, 0] = np.log(0.97)
    ratio = np.array([1.0, 0.55, 1.0], np.float32)[:B]
    return SimpleNamespace(logp=np.ascontiguousarray(logp, np.float32), top=topk_lists(logp, P), ratio=ratio, W=beam, P=P, lp=lp, name=name,
                           key=("make", Tp, beam, pruning, name, lp))


@functools.lru_cache(maxsize=None)
def long_case():
    """The 32-piece phrase held one frame per piece, then its first 8 pieces and another label: it completes once and breaks off at depth 8 once."""
    rng = np.random.RandomState(3)
    path = list(LONG) + list(LONG[:8]) + [IX["▁zz"]]
    x = rng.randn(3, len(path), V).astype(np.float32)
    for t, c in enumerate(path):
        x[:, t, c] += 7.0
    m = x.max(-1, keepdims=True)
    logp = (x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))).astype(np.float32)
    return SimpleNamespace(logp=logp, top=topk_lists(logp, 3), ratio=np.ones(3, np.float32), W=4, P=3, lp=0.0, name="long", key=("long",),
                           path=path)


@functools.lru_cache(maxsize=None)
def ties_case(name="shared_prefix"):
    """Log-posteriors on a grid of quarters and dyadic scores: candidates tie exactly, in score_ctc and in the whole key, and the order
    of the pruned list decides."""
    rng = np.random.RandomState(77)
    B, Tp = 3, 12
    logp = (-rng.randint(1, 9, (B, Tp, V)) / 4.0).astype(np.float32)
    return SimpleNamespace(logp=logp, top=topk_lists(logp, 6), ratio=np.array([1.0, 0.7, 0.3], np.float32), W=5, P=6, lp=0.25, name=name,
                           key=("ties", name))


@functools.lru_cache(maxsize=None)
def repeat_case():
    """Every label of a path through the "doubled" set is held for three frames with a blank only where the phrase doubles a piece: a
    held label must not step the automaton, the doubled piece must."""
    rng = np.random.RandomState(5)
    path = [IX["▁a"], IX["b"], 0, IX["b"], IX["c"], 0, IX["c"], IX["▁b"], IX["c"], 0, IX["c"]]
    x = rng.randn(3, 3 * len(path), V).astype(np.float32)
    for t in range(x.shape[1]):
        x[:, t, path[t // 3]] += 7.0
    m = x.max(-1, keepdims=True)
    logp = (x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))).astype(np.float32)
    return SimpleNamespace(logp=logp, top=topk_lists(logp, 4), ratio=np.ones(3, np.float32), W=4, P=4, lp=0.0, name="doubled", key=("repeat",),
                           labels=[c for c in path if c])


_MODEL = {}


def model_beams(case, gaps=None):
    """The float64 model's beams of a case, computed once (and the gaps of its keys at the keep / drop boundaries)."""
    if case.key not in _MODEL:
        g = []
        _MODEL[case.key] = (model.search(case.logp, case.top, src_sizes(case.ratio, case.logp.shape[1]), case.W, case.lp, SETS[case.name][0],
                                         gaps=g), g)
    if gaps is not None:
        gaps.extend(_MODEL[case.key][1])
    return _MODEL[case.key][0]


def call_args(case, desc, o, cap, blank=0, dev=None):
    """The arguments of cn_ctc_bias_beam_host / cn_op_ctc_bias_beam (without the stream) over numpy arrays, or over the tensors ``dev``."""
    p = dev or SimpleNamespace(logp=case.logp, top=case.top, ratio=case.ratio, **vars(o))
    B, Tp, Vc = case.logp.shape
    return (C.byref(desc), _ptr(p.logp), _ptr(p.top) if case.P else None, _ptr(p.ratio), B, Tp, Vc, case.W, case.P, case.lp, blank, _ptr(p.hyp), cap,
            _ptr(p.hlen), _ptr(p.sc), _ptr(p.slm), _ptr(p.pb), _ptr(p.pnb), _ptr(p.nb))


def run_host(case, bias=None, flavour=None):
    bias = bias or bias_of(case.name)
    B, Tp, _ = case.logp.shape
    cap = Tp + 1
    o = outputs(B, case.W, cap)
    L = hip.lib(flavour)
    rc = L.cn_ctc_bias_beam_host(*call_args(case, bias.desc(), o, cap))
    assert rc == 0, L.cn_last_error()
    assert untouched(o, B, case.W, cap)
    return beams_of(o, B, case.W, cap)
