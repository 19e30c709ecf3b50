"""CTC prefix beam search with phrase biasing, the parts that need no GPU: cn_ctc_bias_beam_host (csrc/ctc_bias_search.h: the serial
loop over the functions the kernel is made of) against tests/ctc_bias_model.py - hypotheses and order exact, score_lm bit for bit
(dyadic scores), score_ctc / p_blk / p_nblk to 1e-8, eight sentinels behind every output untouched -, its refusals, the ABI table,
and the refusals of ctc_beam_decode and of the tasks."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest

import ctc_bias_cases as cases
import ctc_bias_model as model
from cassnat_asr_public_amd import abi, hip
from cassnat_asr_public_amd.models.bias import BiasList
from cassnat_asr_public_amd.models.ngram import _ptr
from cassnat_asr_public_amd.utils.beam_decode import ctc_beam_decode

NEW = ("cn_ctc_beam_bias", "cn_op_ctc_bias_beam", "cn_ctc_bias_beam_host")


def test_entry_points_are_declared_in_a_table_of_their_own_and_exported_by_both_libraries():
    tables = [abi.FUNCTIONS, abi.EXTRA_FUNCTIONS, abi.PROJ_FUNCTIONS, abi.AST_NGRAM_FUNCTIONS, abi.NAT_NGRAM_FUNCTIONS, abi.CTC_TIMES_FUNCTIONS,
              abi.SCORE_FUNCTIONS]
    assert sorted(abi.CTC_BIAS_FUNCTIONS) == sorted(NEW) and not any(set(NEW) & set(t) for t in tables)
    assert "cn_bias_desc" not in abi.STRUCTS and hip.CnBiasDesc is abi.CTC_BIAS_STRUCTS["cn_bias_desc"]
    with open(abi.CTC_BIAS_HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    found = re.findall(r"^([\w \*]+?)\s*\b(cn_\w+)\s*\(([^()]*)\)\s*;", text, re.M)
    assert sorted(name for _, name, _ in found) == sorted(NEW)
    ngram = {"cn_ctc_beam_bias": "cn_ctc_beam_ngram", "cn_op_ctc_bias_beam": "cn_op_ctc_ngram_beam", "cn_ctc_bias_beam_host": "cn_ctc_ngram_beam_host"}
    for flavour in (None, "f16"):
        L = hip.lib(flavour)
        for ret, name, params in found:
            fn = getattr(L, name)
            assert ret.strip() == "int" and fn.restype is C.c_int, name
            assert len(fn.argtypes) == params.count(",") + 1 == len(abi.CTC_BIAS_FUNCTIONS[name][1]), name
            at = 1 if name == "cn_ctc_beam_bias" else 0
            assert fn.argtypes[at] == C.POINTER(hip.CnBiasDesc), name
            # the argument list of the n-gram twin, the descriptor in place of cn_ngram_desc, without lm_scale
            twin = list(abi.EXTRA_FUNCTIONS[ngram[name]][1])
            twin[at] = C.POINTER(hip.CnBiasDesc)
            twin.remove(C.c_double)
            assert list(fn.argtypes) == twin, name
    assert C.sizeof(hip.CnBiasDesc) == 6 * 8 + 4 * 4


@pytest.mark.parametrize("name", list(cases.SETS))
@pytest.mark.parametrize("beam,pruning", cases.BEAMS)
@pytest.mark.parametrize("Tp", cases.SHAPES)
def test_host_search_is_the_model(Tp, beam, pruning, name):
    case = cases.make_case(Tp, beam, pruning, name)
    got, want = cases.run_host(case), cases.model_beams(case)
    cases.same_beams(got, want)
    # the utterance whose every frame is blank: the empty hypothesis, nothing banked
    assert [e["hyp"] for e in got[2]] == [[]] and got[2][0]["score_lm"] == 0.0 and got[2][0]["score_ctc"] == 0.0
    # the one cut short saw frames 0 .. int(0.55 * T') only
    assert all(len(e["hyp"]) <= int(np.float32(0.55) * np.float32(Tp)) + 1 for e in got[1])
    # the invariant: what is left is the rescan of the labels
    phrases = cases.SETS[name][0]
    assert all(e["score_lm"] == model.rescan(e["hyp"], phrases) for seqs in got for e in seqs)
    if pruning * beam >= 32 * 32:
        assert beam * (case.P + 1) > 256


def test_the_f16_library_exports_the_same_search():
    case = cases.make_case(12, 5, 3, "interior")
    cases.same_beams(cases.run_host(case, flavour="f16"), cases.run_host(case), tol=0.0)


def test_the_bonus_decides_something():
    case = cases.make_case(40, 5, 3, "shared_prefix")
    biased, plain = cases.run_host(case), cases.run_host(case, bias=cases.bias_of("none"))
    assert [e["hyp"] for e in biased[0]] != [e["hyp"] for e in plain[0]]
    assert all(e["score_lm"] == 0.0 for seqs in plain for e in seqs) and any(e["score_lm"] > 0 for e in biased[0])


def test_the_32_piece_phrase():
    case = cases.long_case()
    got = cases.run_host(case)
    cases.same_beams(got, cases.model_beams(case))
    assert got[0][0]["hyp"] == case.path and got[0][0]["score_lm"] == 16.0


def test_held_labels_stay_and_the_doubled_piece_steps():
    case = cases.repeat_case()
    got = cases.run_host(case)
    cases.same_beams(got, cases.model_beams(case))
    phrases = cases.SETS["doubled"][0]
    for b in range(3):
        assert got[b][0]["hyp"] == case.labels
        # "▁a b b c" (4 * 2) and "▁b c c" (3 * 3) bank; the "c" between them is left over
        assert got[b][0]["score_lm"] == 8.0 + 9.0 == model.rescan(case.labels, phrases)


@pytest.mark.parametrize("name", ["shared_prefix", "negative", "probe_wrap"])
def test_exact_ties_are_decided_by_list_order(name):
    case = cases.ties_case(name)
    got, want = cases.run_host(case), cases.model_beams(case)
    cases.same_beams(got, want)
    ties = 0
    for seqs in want:
        keys = [e["score_ctc"] + e["score_lm"] + case.lp * len(e["hyp"]) for e in seqs]
        ties += sum(a == b for a, b in zip(keys, keys[1:]))
    assert ties > 0  # kept hypotheses with the same key: only the stable order tells them apart


def test_pruning_zero_needs_no_list():
    case = cases.make_case(12, 2, 0, "one_piece")
    assert case.top.shape[2] == 0
    assert all(e["hyp"] == [] for seqs in cases.run_host(case) for e in seqs)


def test_labels_outside_the_vocabulary_make_no_candidate():
    case = cases.make_case(12, 5, 3, "interior")
    want = cases.run_host(case)
    wide = SimpleNamespace(**vars(case))
    wide.P = 5
    wide.top = np.concatenate([np.full(case.top.shape[:2] + (1,), cases.V, np.int32), case.top,
                               np.full(case.top.shape[:2] + (1,), -3, np.int32)], axis=2)
    cases.same_beams(cases.run_host(wide), want, tol=0.0)


def test_a_descriptor_with_the_root_alone_needs_no_tables():
    case = cases.make_case(12, 5, 3, "none")
    want = cases.run_host(case)
    for nodes in (0, 1):
        d = hip.CnBiasDesc()
        d.slots, d.nodes, d.hash_bits = 1, nodes, 32
        B, Tp, _ = case.logp.shape
        o = cases.outputs(B, case.W, Tp + 1)
        assert hip.lib().cn_ctc_bias_beam_host(*cases.call_args(case, d, o, Tp + 1)) == 0, hip.lib().cn_last_error()
        assert cases.untouched(o, B, case.W, Tp + 1)
        cases.same_beams(cases.beams_of(o, B, case.W, Tp + 1), want, tol=0.0)


def test_refusals_before_any_work():
    L = hip.lib()
    case = cases.make_case(12, 5, 3, "interior")
    B, Tp, V = case.logp.shape
    o = cases.outputs(B, 5, Tp + 1, pad=0)
    good = cases.bias_of("interior").desc()

    def edited(**kw):
        d = hip.CnBiasDesc()
        C.memmove(C.byref(d), C.byref(good), C.sizeof(d))
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(desc=good, logp=_ptr(case.logp), top=_ptr(case.top), ratio=_ptr(case.ratio), B=B, Tp=Tp, V=V, W=5, P=3, lp=0.0, blank=0,
             hyp=_ptr(o.hyp), cap=Tp + 1, hlen=_ptr(o.hlen), slm=_ptr(o.slm), nb=_ptr(o.nb)):
        rc = L.cn_ctc_bias_beam_host(C.byref(desc) if desc is not None else None, logp, top, ratio, B, Tp, V, W, P, lp, blank, hyp, cap, hlen,
                                     _ptr(o.sc), slm, _ptr(o.pb), _ptr(o.pnb), nb)
        return rc, L.cn_last_error()

    for kw, msg in ((dict(desc=None), b"null"), (dict(logp=None), b"null"), (dict(top=None), b"null"), (dict(ratio=None), b"null"),
                    (dict(hyp=None), b"null"), (dict(hlen=None), b"null"), (dict(nb=None), b"null"), (dict(slm=None), b"null"),
                    (dict(W=0), b"ctc_beam"), (dict(W=33), b"ctc_beam"), (dict(P=-1), b"ctc_pruning"), (dict(P=33), b"ctc_pruning"),
                    (dict(desc=edited(slots=good.slots - 1)), b"power of two"), (dict(desc=edited(slots=0)), b"power of two"),
                    (dict(desc=edited(nodes=-1)), b"negative"), (dict(desc=edited(hash_bits=33)), b"hash_bits"),
                    (dict(desc=edited(hash_bits=-1)), b"hash_bits"),
                    (dict(desc=edited(fail=None)), b"null table"), (dict(desc=edited(edge_keys=None)), b"null table"),
                    (dict(desc=edited(edge_child=None)), b"null table"), (dict(desc=edited(value=None)), b"null table"),
                    (dict(desc=edited(bank=None)), b"null table"), (dict(desc=edited(reset=None)), b"null table"),
                    (dict(B=0), b"positive"), (dict(Tp=0), b"positive"), (dict(V=0), b"positive"),
                    (dict(blank=-1), b"blank"), (dict(blank=V), b"blank"), (dict(cap=Tp), b"hyp_cap"),
                    (dict(lp=float("nan")), b"number")):
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
    for a, s in ((o.hyp, cases.SENT_I), (o.hlen, cases.SENT_I), (o.nb, cases.SENT_I), (o.sc, cases.SENT_F), (o.slm, cases.SENT_F),
                 (o.pb, cases.SENT_F), (o.pnb, cases.SENT_F)):
        assert (a == s).all()
    assert call()[0] == 0 and (o.nb[:B] >= 1).all()
    # the device entries refuse the same arguments before they touch the GPU
    assert L.cn_op_ctc_bias_beam(C.byref(good), _ptr(case.logp), _ptr(case.top), _ptr(case.ratio), B, Tp, V, 33, 3, 0.0, 0, _ptr(o.hyp), Tp + 1,
                                 _ptr(o.hlen), _ptr(o.sc), _ptr(o.slm), _ptr(o.pb), _ptr(o.pnb), _ptr(o.nb), None) != 0
    assert b"ctc_beam" in L.cn_last_error()
    assert L.cn_op_ctc_bias_beam(C.byref(edited(slots=3)), _ptr(case.logp), _ptr(case.top), _ptr(case.ratio), B, Tp, V, 5, 3, 0.0, 0, _ptr(o.hyp),
                                 Tp + 1, _ptr(o.hlen), _ptr(o.sc), _ptr(o.slm), _ptr(o.pb), _ptr(o.pnb), _ptr(o.nb), None) != 0
    assert b"power of two" in L.cn_last_error()
    assert L.cn_ctc_beam_bias(None, C.byref(good), None, None, 2, 61, 80, None, 5, 8, 0.2, None, 17, None, None, None, None, None, None, None) != 0
    assert L.cn_last_error()


# ---- ctc_beam_decode and the tasks ---------------------------------------------------------------------------------------------------
def test_a_bias_list_with_a_fused_language_model_is_refused_before_any_device_call():
    bias = cases.bias_of("interior")
    lm = SimpleNamespace(step_engine=lambda n: None)
    for kw, args in ((dict(bias=bias), SimpleNamespace(ctc_lm_weight=0.3)), (dict(), SimpleNamespace(ctc_lm_weight=0.3, hip_bias_model=bias))):
        with pytest.raises(NotImplementedError, match="hip_bias"):
            ctc_beam_decode(None, None, None, None, None, args, lm, **kw)  # (model, features and vocabulary are None: nothing was touched)


@pytest.mark.parametrize("task,decode_type,extra,names", [("cassnat", "att_only", dict(), "att_only"), ("cassnat", "att_only", dict(sample_num=4), "ESA"),
                                                          ("art", "ctc_att", dict(), "ctc_att"), ("art", "ctc_correct", dict(), "ctc_correct")])
def test_tasks_refuse_the_flag_on_paths_without_the_search(task, decode_type, extra, names):
    from cassnat_asr_public_amd.tasks import ArtTask, CassNATTask

    cls = CassNATTask if task == "cassnat" else ArtTask
    self = cls.__new__(cls)  # (decode looks at the arguments before it touches the loader or the model)
    self.test_loader = []
    args = SimpleNamespace(decode_type=decode_type, hip_bias="list.txt", hip_bias_model=None, beam_width=1, **extra)
    with pytest.raises(NotImplementedError, match="hip_bias") as e:
        cls.decode(self, args)
    assert names in str(e.value)


def test_the_parser_knows_the_flags():
    from cassnat_asr_public_amd.utils.parser import DecodeParser

    base = ["--task", "cassnat", "--test_config", "c.yaml", "--data_path", "f.scp", "--resume_model", "m.mdl", "--result_file", "r.txt"]
    a = DecodeParser().get_args(base)
    assert a.hip_bias == "" and a.hip_bias_score == 3.0
    a = DecodeParser().get_args(base + ["--hip_bias", "names.txt", "--hip_bias_score", "1.5"])
    assert a.hip_bias == "names.txt" and a.hip_bias_score == 1.5
