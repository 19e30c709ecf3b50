"""CTC prefix beam search with word n-gram fusion, the parts that need no GPU: cn_ctc_ngram_beam_host (csrc/ctc_ngram_search.h: the
serial loop over the functions the kernel is made of) against tests/ctc_ngram_model.py - hypotheses and order exact, score_lm bit for
bit on dyadic models, score_ctc / p_blk / p_nblk to 1e-8 -, its refusals, and ctc_beam_decode's refusals of a kenlm-like object and
of an NgramLM whose vocabulary cannot be glued."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import ctc_ngram_cases as cases
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.models.ngram import NgramLM, _ptr
from cassnat_asr_public_amd.utils.beam_decode import ctc_beam_decode
from ctc_ngram_model import search
from ngram_model import text_of

NEW = ("cn_ctc_beam_ngram", "cn_op_ctc_ngram_beam", "cn_ctc_ngram_beam_host")


def model_beams(case):
    _, model = cases.lm_of(case.order, case.hash_bits)
    return search(case.logp, case.top, cases.src_sizes(case.ratio, case.logp.shape[1]), case.W, case.lp, case.lm_scale, model, cases.VOCAB)


def test_entry_points_are_declared_and_exported_by_both_libraries():
    """include/cassnat_hip_ctc_ngram.h, the companion of cassnat_hip.h, declares them; the parser that reads the main header reads it
    and both libraries are bound from it.  Parameter counts and return types are counted from the header's text here."""
    import re

    from cassnat_asr_public_amd import abi

    assert sorted(abi.EXTRA_FUNCTIONS) == sorted(NEW) and not set(NEW) & set(abi.FUNCTIONS)
    with open(abi.EXTRA_HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    found = re.findall(r"^([\w \*]+?)\s*\b(cn_\w+)\s*\(([^()]*)\)\s*;", text, re.M)
    assert sorted(name for _, name, _ in found) == sorted(NEW)
    for flavour in (None, "f16"):
        L = hip.lib(flavour)
        for ret, name, params in found:
            fn = getattr(L, name)
            assert ret.strip() == "int" and fn.restype is C.c_int, name
            assert len(fn.argtypes) == params.count(",") + 1 == len(abi.EXTRA_FUNCTIONS[name][1]), name
            assert fn.argtypes[1 if name == "cn_ctc_beam_ngram" else 0] == C.POINTER(hip.CnNgramDesc), name


@pytest.mark.parametrize("order", cases.ORDERS)
@pytest.mark.parametrize("beam,pruning", cases.BEAMS)
@pytest.mark.parametrize("Tp", cases.SHAPES)
def test_host_search_is_the_model(Tp, beam, pruning, order):
    case = cases.make_case(Tp, beam, pruning, order)
    got, want = cases.run_host(case), model_beams(case)
    cases.same_beams(got, want)
    # the utterance whose every frame is blank: the empty hypothesis with </s> alone
    _, model = cases.lm_of(order)
    assert [e["hyp"] for e in got[2]] == [[]] and got[2][0]["score_lm"] == case.lm_scale * model.score("")[0] and got[2][0]["score_ctc"] == 0.0
    # the one cut short saw frames 0 .. int(0.55 * T') only
    assert all(len(e["hyp"]) <= int(np.float32(0.55) * np.float32(Tp)) + 1 for e in got[1])


def test_beams_close_words_in_mid_search():
    case = cases.make_case(40, 5, 3, 3)
    got = cases.run_host(case)
    texts = [text_of(e["hyp"], len(e["hyp"]), cases.VOCAB) for e in got[0]]
    assert max(len(t.split()) for t in texts) >= 4, texts
    _, model = cases.lm_of(3)
    for e, t in zip(got[0], texts):  # the invariant: lm_scale times the sum of the word scores, exactly on a dyadic model
        assert e["score_lm"] == case.lm_scale * model.score(t)[0]
    # and the LM decides something: another lm_scale, another beam
    other = cases.run_host(cases.make_case(40, 5, 3, 3, lm_scale=4.0))
    assert [e["hyp"] for e in other[0]] != [e["hyp"] for e in got[0]]


def test_repetitions_do_not_append_the_last_label_again():
    case = cases.repeat_case()
    got = cases.run_host(case)
    cases.same_beams(got, model_beams(case))
    for b in range(3):
        assert got[b][0]["hyp"] == case.path, got[b][0]["hyp"]
    assert all((case.top[:, t] == case.path[t // 3]).any() for t in range(18))  # the label held is among the pruned ones


@pytest.mark.parametrize("order", [1, 3])
def test_exact_ties_are_decided_by_list_order(order):
    case = cases.ties_case(order)
    got, want = cases.run_host(case), model_beams(case)
    cases.same_beams(got, want)
    ties = 0
    for seqs in want:
        keys = [e["score_ctc"] + e["score_lm"] + case.lp * len(e["hyp"]) for e in seqs]
        ties += sum(a == b for a, b in zip(keys, keys[1:]))
    assert ties > 0  # kept hypotheses with the same key: only the stable order tells them apart


def test_colliding_word_keys():
    case = cases.collision_case()
    assert case.hash_bits < 64 and case.hit
    got, want = cases.run_host(case), model_beams(case)
    cases.same_beams(got, want)
    _, told = cases.lm_of(1, case.hash_bits)
    _, untold = cases.lm_of(1)
    words = [w for seqs in got for e in seqs for w in text_of(e["hyp"], len(e["hyp"]), cases.VOCAB).split()]
    taken = [w for w in words if w not in cases.WORDS and told.alias(w) != w]
    assert taken, (case.hit, words)  # a word outside the model was taken for one of the model's
    assert any(e["score_lm"] != case.lm_scale * untold.score(text_of(e["hyp"], len(e["hyp"]), cases.VOCAB))[0] for seqs in got for e in seqs)


def test_pruning_zero_needs_no_list():
    case = cases.make_case(12, 2, 0, 2)
    assert case.top.shape[2] == 0
    got = cases.run_host(case)
    assert all(e["hyp"] == [] for seqs in got for e in seqs)


def test_labels_outside_the_vocabulary_make_no_candidate():
    case = cases.make_case(12, 5, 3, 2)
    want = cases.run_host(case)
    wide = SimpleNamespace(**vars(case))
    wide.P = 5
    wide.top = np.concatenate([np.full(case.top.shape[:2] + (1,), cases.V, np.int32), case.top,
                               np.full(case.top.shape[:2] + (1,), -3, np.int32)], axis=2)
    cases.same_beams(cases.run_host(wide), want, tol=0.0)


def test_refusals_before_any_work():
    L = hip.lib()
    lm, _ = cases.lm_of(3)
    case = cases.make_case(12, 5, 3, 3)
    B, Tp, V = case.logp.shape
    o = cases.outputs(B, 5, Tp + 1, pad=0)
    good = lm.desc()

    def edited(**kw):
        d = hip.CnNgramDesc()
        C.memmove(C.byref(d), C.byref(good), C.sizeof(d))
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(desc=good, logp=_ptr(case.logp), top=_ptr(case.top), ratio=_ptr(case.ratio), B=B, Tp=Tp, V=V, W=5, P=3, lp=0.0, scale=0.5, blank=0,
             hyp=_ptr(o.hyp), cap=Tp + 1, hlen=_ptr(o.hlen), nb=_ptr(o.nb)):
        rc = L.cn_ctc_ngram_beam_host(C.byref(desc) if desc is not None else None, logp, top, ratio, B, Tp, V, W, P, lp, scale, blank, hyp, cap,
                                      hlen, _ptr(o.sc), _ptr(o.slm), _ptr(o.pb), _ptr(o.pnb), nb)
        return rc, L.cn_last_error()

    for kw, msg in ((dict(desc=None), b"null"), (dict(logp=None), b"null"), (dict(top=None), b"null"), (dict(ratio=None), b"null"),
                    (dict(hyp=None), b"null"), (dict(hlen=None), b"null"), (dict(nb=None), b"null"),
                    (dict(W=0), b"ctc_beam"), (dict(W=33), b"ctc_beam"), (dict(P=-1), b"ctc_pruning"), (dict(P=33), b"ctc_pruning"),
                    (dict(desc=edited(order=0)), b"order"), (dict(desc=edited(order=9)), b"order"),
                    (dict(desc=edited(gram_slots=good.gram_slots - 1)), b"powers of two"), (dict(desc=edited(word_slots=0)), b"powers of two"),
                    (dict(desc=edited(gram_bo=None)), b"null table"), (dict(desc=edited(vocab=-1)), b"vocab"),
                    (dict(B=0), b"positive"), (dict(Tp=0), b"positive"), (dict(V=0), b"positive"),
                    (dict(blank=-1), b"blank"), (dict(blank=V), b"blank"), (dict(cap=Tp), b"hyp_cap"),
                    (dict(scale=float("nan")), b"numbers"), (dict(lp=float("nan")), b"numbers")):
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
    for a, s in ((o.hyp, cases.SENT_I), (o.hlen, cases.SENT_I), (o.nb, cases.SENT_I), (o.sc, cases.SENT_F), (o.slm, cases.SENT_F),
                 (o.pb, cases.SENT_F), (o.pnb, cases.SENT_F)):
        assert (a == s).all()
    assert call()[0] == 0 and (o.nb[:B] >= 1).all()
    # the device entries refuse the same arguments before they touch the GPU
    assert L.cn_op_ctc_ngram_beam(C.byref(good), _ptr(case.logp), _ptr(case.top), _ptr(case.ratio), B, Tp, V, 33, 3, 0.0, 0.5, 0, _ptr(o.hyp),
                                  Tp + 1, _ptr(o.hlen), _ptr(o.sc), _ptr(o.slm), _ptr(o.pb), _ptr(o.pnb), _ptr(o.nb), None) != 0
    assert b"ctc_beam" in L.cn_last_error()
    assert L.cn_ctc_beam_ngram(None, C.byref(good), None, None, 2, 61, 80, None, 5, 8, 0.2, 0.3, None, 17, None, None, None, None, None, None,
                               None) != 0
    assert L.cn_last_error()


# ---- ctc_beam_decode ---------------------------------------------------------------------------------------------------------------
def test_a_kenlm_like_object_is_refused_with_both_accepted_types_named():
    for lm_model in (SimpleNamespace(score=lambda text: 0.0), object()):
        with pytest.raises(NotImplementedError, match="in-loop LM fusion") as e:
            ctc_beam_decode(None, None, None, None, None, None, lm_model)
        assert "TransformerLM" in str(e.value) and "NgramLM" in str(e.value)


def test_an_ngram_lm_whose_pieces_cannot_be_glued_is_refused_before_any_device_call(tmp_path):
    from test_ngram_host import SPECIALS, WORKED, vocab_of, write

    lm = NgramLM.load(write(tmp_path, WORKED), vocab_of(SPECIALS + ["▁a", "a▁b", "▁b"]))
    assert not lm.device_ok
    args = SimpleNamespace(ctc_lm_weight=0.3)
    with pytest.raises(ValueError, match="separator"):
        ctc_beam_decode(None, None, None, None, None, args, lm)  # (model, features and vocabulary are None: nothing was touched)
