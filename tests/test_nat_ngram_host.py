"""CASS-NAT finish loop with word n-gram fusion, the parts that need no GPU: the companion header and its binding, the refusals of the
entry points, the host entry cn_nat_ngram_finish_host against the numpy model (tests/nat_ngram_model.py), and the admissions and
refusals of CassNATTask.load_lm_model and CassNAT._check_args."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest

import nat_ngram_cases as cases
import nat_ngram_model as nn
from cassnat_asr_public_amd import abi, hip, synth
from cassnat_asr_public_amd.models import make_cassnat_model
from cassnat_asr_public_amd.models.lm import TransformerLM
from cassnat_asr_public_amd.models.ngram import NgramLM, _ptr
from cassnat_asr_public_amd.tasks.cassnat_task import CassNATTask
from ngram_model import random_arpa

V = 40


def test_entry_points_are_declared_in_the_new_header_only_and_exported_by_both_libraries():
    assert sorted(abi.NAT_NGRAM_FUNCTIONS) == sorted(cases.NEW)
    assert not set(cases.NEW) & (set(abi.FUNCTIONS) | set(abi.EXTRA_FUNCTIONS) | set(abi.PROJ_FUNCTIONS) | set(abi.AST_NGRAM_FUNCTIONS))
    with open(abi.NAT_NGRAM_HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    found = re.findall(r"^([\w \*]+?)\s*\b(cn_\w+)\s*\(([^()]*)\)\s*;", text, re.M)
    assert sorted(name for _, name, _ in found) == sorted(cases.NEW)
    for flavour in (None, "f16"):
        L = hip.lib(flavour)
        for ret, name, params in found:
            fn = getattr(L, name)
            assert ret.strip() == "int" and fn.restype is C.c_int, name
            assert len(fn.argtypes) == params.count(",") + 1 == len(abi.NAT_NGRAM_FUNCTIONS[name][1]), name
    # the older headers keep their lists, the option structs their sizes
    assert len(abi.FUNCTIONS) == 121 and len(abi.EXTRA_FUNCTIONS) == 3 and len(abi.AST_NGRAM_FUNCTIONS) == 6
    assert C.sizeof(hip.CnDecodeOpts) == 64 and C.sizeof(hip.CnAstOpts) == 56


def test_null_and_geometry_refusals():
    L = hip.lib()
    lm, _ = cases.lm_for(3, V)
    assert L.cn_nat_attach_ngram(None, C.byref(lm.desc()), 0.5) != 0
    assert b"cfg.ast = 0" in L.cn_last_error()
    assert L.cn_nat_ngram_finish(None, None, 3, 3, 2, 1, 0.0, 0, None, 4, None, None, None) != 0
    assert b"null argument" in L.cn_last_error()
    assert L.cn_op_nat_class_topk(None, None, None, 2, 5, 40, None, 2, 3, None, None, None, None) != 0
    assert b"null argument" in L.cn_last_error()
    assert L.cn_op_nat_ngram_finish(None, 0.5, None, None, None, None, 2, 5, 3, 2, 1, 0, 1, 0.0, None, None, 6, None, None, None) != 0
    assert b"null argument" in L.cn_last_error()
    att, ylen = cases.rows_of(2, 4, V), np.array([4, 2], np.int32)
    hyp, hlen, sc = np.zeros(2 * 3 * 5, np.int32), np.zeros(6, np.int32), np.zeros(6)

    def host(desc=lm.desc(), att=att, B=2, U=4, Vv=V, ymax=4, bw=3, eos=cases.EOS, Lm=5, scale=0.5, lp=0.0):
        return L.cn_nat_ngram_finish_host(C.byref(desc) if desc is not None else None, scale, _ptr(att) if att is not None else None, _ptr(ylen), None,
                                          B, U, Vv, ymax, bw, eos, cases.SOS, cases.PAD, 1, lp, _ptr(hyp), Lm, _ptr(hlen), _ptr(sc))

    def changed(**kw):
        d = hip.CnNgramDesc.from_buffer_copy(lm.desc())
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert host() == 0
    for kw, what in ((dict(desc=None), "null"), (dict(att=None), "null"), (dict(B=0), "positive"), (dict(U=0), "positive"),
                     (dict(Vv=8193), "8192"), (dict(bw=0), "beam_width"), (dict(bw=17), "beam_width"), (dict(bw=41), "beam_width"),
                     (dict(eos=-1), "eos"), (dict(eos=V), "eos"), (dict(ymax=0), "ymax"), (dict(ymax=5), "ymax"), (dict(Lm=4), "max_len"),
                     (dict(Vv=39), "vocabulary"), (dict(scale=float("nan")), "numbers"), (dict(lp=float("nan")), "numbers"),
                     (dict(desc=changed(order=0)), "order 0 is outside 1 .. 8"), (dict(desc=changed(order=9)), "order 9 is outside 1 .. 8"),
                     (dict(desc=changed(gram_slots=48)), "powers of two"), (dict(desc=changed(piece_starts=None)), "null table")):
        assert host(**kw) != 0 and what in L.cn_last_error().decode(), (kw, L.cn_last_error())


@pytest.mark.parametrize("order", [1, 2, 3, 5])
@pytest.mark.parametrize("bw,U", [(1, 5), (3, 1), (3, 7), (16, 5)])
def test_host_entry_is_the_model(order, bw, U):
    """Hypotheses, their order and the float64 scores exact, on a dyadic model: planted rows and rows on a grid of quarters (exact ties
    in att and in the fused values), with and without the length penalty, with rows past ylen read as zero."""
    lm, model = cases.lm_for(order, V)
    vocab = cases.vocab_of(V)
    ylen = cases.lens_of(3, U)
    for grid in (False, True):
        att = cases.rows_of(3, U, V, seed=order, grid=grid)
        for lp, zero in ((0.25, False), (None, True)):
            got = cases.run_host(lm, att, ylen, U, bw, 0.5, lp=lp or 0.0, use_lp=int(lp is not None), zlen=ylen if zero else None)
            want = nn.finish(att, ylen, U, model, vocab, cases.EOS, bw, 0.5, lp, cases.SOS, cases.PAD, zero_past_len=zero)
            cases.same_beams(got, want)
    assert [len(u[0]["hyp"]) for u in got] == [min(int(n), U - 1) + 2 for n in ylen]


def test_host_entry_on_a_model_that_rounds_and_with_a_shorter_ymax():
    lm, model = cases.plain_lm(V)
    vocab = cases.vocab_of(V)
    att, ylen = cases.rows_of(3, 9, V, seed=3), np.array([9, 2, 6], np.int32)
    scale = float(np.float32(0.3 * np.log(10.0)))
    trace = []
    want = nn.finish(att, ylen, 5, model, vocab, cases.EOS, 4, scale, 0.1, cases.SOS, cases.PAD, trace=trace)
    cases.same_beams(cases.run_host(lm, att, ylen, 5, 4, scale, lp=0.1, L=9), want)   # ymax < U, max_len > ymax + 1
    assert any(a[0] != 0 for *_, a in trace) and all(a[1] != 0 for *_, a in trace)     # words were closed; eos always costs
    free = nn.finish(att, ylen, 5, model, vocab, cases.EOS, 4, 0.0, 0.1, cases.SOS, cases.PAD)
    assert any(w[0]["hyp"] != f[0]["hyp"] for w, f in zip(want, free))                 # the model decides something


def test_host_entry_with_colliding_word_keys():
    (lm, model), case = cases.collision_lm(V)
    vocab = cases.vocab_of(V)
    att, ylen = cases.spelled_rows(case.hit[:4], V)
    U = att.shape[1]
    got = cases.run_host(lm, att, ylen, U, 5, 0.5, lp=0.1)
    cases.same_beams(got, nn.finish(att, ylen, U, model, vocab, cases.EOS, 5, 0.5, 0.1, cases.SOS, cases.PAD))
    _, untold = cases.lm_for(1, V)
    other = nn.finish(att, ylen, U, untold, vocab, cases.EOS, 5, 0.5, 0.1, cases.SOS, cases.PAD)
    assert [[e["score"] for e in u] for u in got] != [[e["score"] for e in u] for u in other]  # a word outside the model was taken for one of it


# ---- CassNATTask.load_lm_model / CassNAT._check_args --------------------------------------------------------------------------------
def _task():
    return SimpleNamespace(vocab=cases.vocab_of(V), lm_model=None)


def test_load_lm_model_loads_an_arpa_text_for_lm_weight(tmp_path):
    path = tmp_path / "m.arpa"
    path.write_text(random_arpa(cases.WORDS, 3, seed=4), encoding="utf-8")
    task = _task()
    args = SimpleNamespace(lm_weight=0.5, ctc_lm_weight=0, rank_model="n-gram", rnnlm=str(path), lm_config=None)
    CassNATTask.load_lm_model(task, args)
    assert isinstance(task.lm_model, NgramLM) and task.lm_model.order == 3 and task.lm_model.vocab_size == V
    args.lm_weight = 0
    CassNATTask.load_lm_model(task, args)
    assert task.lm_model is None


def test_load_lm_model_still_refuses_what_is_no_arpa_text(tmp_path):
    path = tmp_path / "m.bin"
    path.write_bytes(b"mmap lm http://kheafield.com/code format version 5\n\0\0\0\0")
    for rank in ("n-gram", "at_baseline"):
        args = SimpleNamespace(lm_weight=0.5, ctc_lm_weight=0, rank_model=rank, rnnlm=str(path), lm_config=None)
        with pytest.raises(NotImplementedError, match="rank_model 'lm'"):
            CassNATTask.load_lm_model(_task(), args)


def _model(**over):
    args = synth.make_args("tiny", **over)
    return make_cassnat_model(args.input_size, args), args


def test_check_args_admits_an_ngram_model_and_keeps_the_refusals():
    lm, _ = cases.lm_for(3, V)
    for ok in (dict(), dict(beam_width=1), dict(beam_width=16), dict(use_trigger=False), dict(decode_type="ctc_att", sample_num=1),
               dict(sample_num=4, rank_model="n-gram")):
        model, args = _model(**dict(dict(lm_weight=0.6, beam_width=3, rank_model="n-gram"), **ok))
        model._check_args(args, lm)
    model, args = _model(lm_weight=0.6, beam_width=3, sample_num=4, rank_model="lm")
    with pytest.raises(NotImplementedError, match="rank_model 'n-gram'"):
        model._check_args(args, lm)                           # ESA ranks with the model it fuses
    model, args = _model(lm_weight=0.6, beam_width=17)
    with pytest.raises(NotImplementedError, match="beam_width"):
        model._check_args(args, lm)
    model, args = _model(lm_weight=0.6, beam_width=3, decode_type="ctc_att", sample_num=4, rank_model="n-gram")
    with pytest.raises(NotImplementedError, match="ctc_att with sample_num > 1"):
        model._check_args(args, lm)
    model, args = _model(lm_weight=0.6, beam_width=3, test_hitrate=True)
    with pytest.raises(NotImplementedError, match="test_hitrate"):
        model._check_args(args, lm)
    bad = NgramLM.__new__(NgramLM)
    bad.device_ok = False
    model, args = _model(lm_weight=0.6, beam_width=3)
    with pytest.raises(NotImplementedError, match="separator"):
        model._check_args(args, bad)
    # a kenlm-like object, an at_baseline ranker, and a ranker that is neither kind
    kenlm_like, ranker = SimpleNamespace(score=lambda text: 0.0), SimpleNamespace(teacher_score=lambda *a: None)
    model, args = _model(lm_weight=0.6, beam_width=3, sample_num=4, rank_model="n-gram")
    with pytest.raises(NotImplementedError, match="n-gram"):
        model._check_args(args, kenlm_like)
    model, args = _model(lm_weight=0.6, beam_width=3, sample_num=4, rank_model="at_baseline")
    with pytest.raises(NotImplementedError, match="at_baseline"):
        model._check_args(args, ranker)
    model, args = _model(lm_weight=0.6, beam_width=3)
    with pytest.raises(NotImplementedError, match="TransformerLM"):
        model._check_args(args, ranker)
    model._check_args(args, TransformerLM(synth.make_args_lm("tiny_lm", vocab_size=40)))
