"""Inputs shared by tests/test_ctc_merge_model.py, tests/test_ctc_merge_host.py and tests/test_gpu_ctc_merge_kernel.py: the three fusion
policies over the existing case modules' vocabulary, n-gram model and phrase set, the cases (log-posteriors, pruned lists, size ratios
and search settings), the float64 model's result per (case, policy), computed once, and the host entry as a function."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np

import ctc_bias_cases
import ctc_merge_model as model
import ctc_ngram_cases
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.models.ngram import _ptr
from ctc_ngram_cases import SENT_F, SENT_I, beams_of, outputs, same_beams, src_sizes, untouched  # noqa: F401
from ctc_ngram_model import topk_lists

IX, V, VOCAB = ctc_bias_cases.IX, ctc_bias_cases.V, ctc_bias_cases.VOCAB
POLICIES = ("none", "ngram", "bias")
SHAPES = (1, 12, 40)                                    # T'
BEAMS = ((1, 3), (3, 0), (5, 8), (20, 30), (32, 32))    # (ctc_beam, ctc_pruning); pruning is clipped to V - 1 labels: 32 * 28 > 256 candidates
ORDER, LM_SCALE, PHRASES = 3, 0.5, "shared_prefix"      # the n-gram policy's model and the bias policy's list
ABC = (IX["▁a"], IX["b"], IX["c"])
RELINK_SEED = 27  # alphabet_case(12, 3, 3, seed): the smallest seed whose first utterance drops a prefix and makes it again (asserted)


def scorer_of(policy):
    if policy == "ngram":
        return model.NgramScorer(ctc_ngram_cases.lm_of(ORDER)[1], VOCAB, LM_SCALE)
    if policy == "bias":
        return model.BiasScorer(ctc_bias_cases.SETS[PHRASES][0])
    return None


def log_softmax(x):
    m = x.max(-1, keepdims=True)
    return np.ascontiguousarray(x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True))), np.float32)


@functools.lru_cache(maxsize=None)
def make_case(Tp, beam, pruning, lp=0.25):
    """ctc_bias_cases.make_case: 3 utterances - one searched over all its frames, one cut short by its size ratio, one whose every
    frame is blank (skipped)."""
    c = ctc_bias_cases.make_case(Tp, beam, pruning, PHRASES, lp=lp)
    return SimpleNamespace(logp=c.logp, top=c.top, ratio=c.ratio, W=c.W, P=c.P, lp=lp, key=("make", Tp, beam, pruning, lp))


@functools.lru_cache(maxsize=None)
def alphabet_case(Tp, beam, pruning, seed=0, labels=ABC, scale=2.0, lp=0.0, B=3):
    """Blank and a few labels share the mass (every other label far below): the beam can only spell sequences over the few, so nearly
    every frame has an extension that spells a kept hypothesis.  The second utterance is cut short by its size ratio."""
    rng = np.random.RandomState(seed)
    x = np.full((B, Tp, V), -12.0, np.float32) + 0.01 * rng.rand(B, Tp, V).astype(np.float32)
    x[:, :, [0] + list(labels)] = rng.randn(B, Tp, 1 + len(labels)).astype(np.float32) * scale
    logp = log_softmax(x)
    P = min(pruning, V - 1)
    ratio = np.array([1.0, 0.6, 1.0], np.float32)[:B]
    return SimpleNamespace(logp=logp, top=topk_lists(logp, P), ratio=ratio, W=beam, P=P, lp=lp, key=("abc", Tp, beam, pruning, seed, labels, scale, lp))


@functools.lru_cache(maxsize=None)
def runs_case():
    """Runs of one label: "c c c" spelled as c, blank, c, blank, c with every label held two frames, beside "c c" and "c": the
    extension's label equals its parent's last label (c == last) and the kept hypotheses differ only in how many c they have."""
    rng = np.random.RandomState(11)
    c, a = IX["c"], IX["▁a"]
    path = [a, a, c, c, 0, c, c, 0, c, c, a, 0, c, c]
    x = rng.randn(3, len(path), V).astype(np.float32) * 0.5
    for t, lab in enumerate(path):
        x[:, t, lab] += 3.0
        x[1:, t, 0] += 1.5  # (the other utterances are less sure about the second blank: "c c" and "c c c" compete)
    logp = log_softmax(x)
    return SimpleNamespace(logp=logp, top=topk_lists(logp, 4), ratio=np.ones(3, np.float32), W=6, P=4, lp=0.0, key=("runs",),
                           labels=[a, c, c, c, a, c])


@functools.lru_cache(maxsize=None)
def relink_case():
    """A prefix is dropped from the beam while its extension stays, and a later frame makes it again: the extension of the new
    hypothesis must fold into the old one's, though no slot link joins them."""
    return alphabet_case(12, 3, 3, seed=RELINK_SEED)


@functools.lru_cache(maxsize=None)
def duplicate_case():
    """Hand-made pruned lists that name a label twice (and the blank, and ids outside the vocabulary)."""
    base = alphabet_case(12, 5, 3, seed=2)
    top = np.concatenate([base.top[:, :, :2], base.top[:, :, :1], np.full(base.top.shape[:2] + (1,), V, np.int32), base.top[:, :, 2:],
                          base.top[:, :, 1:2], np.zeros(base.top.shape[:2] + (1,), np.int32)], axis=2).astype(np.int32)
    return SimpleNamespace(logp=base.logp, top=np.ascontiguousarray(top), ratio=base.ratio, W=5, P=top.shape[2], lp=0.1, key=("dup",))


def crafted(name):
    return {"abc40": lambda: alphabet_case(40, 5, 8), "abc40_wide": lambda: alphabet_case(40, 32, 32, seed=1), "runs": runs_case,
            "relink": relink_case, "duplicate": duplicate_case, "abc_lp": lambda: alphabet_case(12, 4, 3, seed=5, lp=0.5)}[name]()


CRAFTED = ("abc40", "abc40_wide", "runs", "relink", "duplicate", "abc_lp")
_MODEL = {}


def model_beams(case, policy, merge=True, stats=None):
    """The float64 model's beams of a case under a policy, computed once."""
    key = (case.key, policy, merge)
    if key not in _MODEL:
        st = {}
        _MODEL[key] = (model.search(case.logp, case.top, src_sizes(case.ratio, case.logp.shape[1]), case.W, case.lp, scorer_of(policy),
                                    merge=merge, stats=st), st)
    if stats is not None:
        stats.update(_MODEL[key][1])
    return _MODEL[key][0]


def descs(policy, dev=None):
    """(ngram desc or None, lm_scale, bias desc or None, keep-alive) of a policy; ``dev`` true: tables on the current device."""
    if policy == "ngram":
        lm = ctc_ngram_cases.lm_of(ORDER)[0]
        return lm.cuda().desc(lm.device) if dev else lm.desc(), LM_SCALE, None, lm
    if policy == "bias":
        bias = ctc_bias_cases.bias_of(PHRASES)
        return None, 0.0, bias.cuda().desc(bias.device) if dev else bias.desc(), bias
    return None, 0.0, None, None


def call_args(case, policy, o, cap, blank=0, dev=None, tables=None):
    """The arguments of cn_ctc_merged_beam_host / cn_op_ctc_merged_beam (without the stream) over numpy arrays, or over the tensors
    ``dev`` with the tables on the device ``tables``.  Returns (args, keep-alive)."""
    ng, scale, bias, keep = descs(policy, tables)
    p = dev or SimpleNamespace(logp=case.logp, top=case.top, ratio=case.ratio, **vars(o))
    B, Tp, Vc = case.logp.shape
    return ((C.byref(ng) if ng is not None else None, scale, C.byref(bias) if bias is not None else None, _ptr(p.logp),
             _ptr(p.top) if case.P else None, _ptr(p.ratio), B, Tp, Vc, case.W, case.P, case.lp, blank, _ptr(p.hyp), cap, _ptr(p.hlen),
             _ptr(p.sc), _ptr(p.slm), _ptr(p.pb), _ptr(p.pnb), _ptr(p.nb)), (ng, bias, keep))


_HOST = {}


def run_host(case, policy, flavour=None):
    """cn_ctc_merged_beam_host's beams of a case under a policy (the default library's are computed once)."""
    if flavour is None and (case.key, policy) in _HOST:
        return _HOST[(case.key, policy)]
    B, Tp, _ = case.logp.shape
    cap = Tp + 1
    o = outputs(B, case.W, cap)
    L = hip.lib(flavour)
    args, keep = call_args(case, policy, o, cap)
    rc = L.cn_ctc_merged_beam_host(*args)
    assert rc == 0, L.cn_last_error()
    assert untouched(o, B, case.W, cap)
    got = beams_of(o, B, case.W, cap)
    if flavour is None:
        _HOST[(case.key, policy)] = got
    return got
