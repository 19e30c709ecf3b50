"""The merging CTC prefix beam search, the parts that need no GPU: cn_ctc_merged_beam_host (csrc/ctc_merge_search.h: the serial loop
over the functions the kernel is made of, identity by label vectors) against tests/ctc_merge_model.py under the three fusion policies
- hypotheses and order exact, score_lm bit for bit (dyadic model and scores), score_ctc / p_blk / p_nblk to 1e-8, eight sentinels
behind every output untouched -, its refusals, the ABI table, the parser flag, and the refusals of ctc_beam_decode and of the tasks."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest

import ctc_bias_cases
import ctc_merge_cases as cases
import ctc_ngram_cases
from cassnat_asr_public_amd import abi, hip
from cassnat_asr_public_amd.models.ngram import _ptr
from cassnat_asr_public_amd.utils.beam_decode import ctc_beam_decode

NEW = ("cn_ctc_beam_merged", "cn_op_ctc_merged_beam", "cn_ctc_merged_beam_host")


def test_entry_points_are_declared_in_a_table_of_their_own_and_exported_by_both_libraries():
    tables = [abi.FUNCTIONS, abi.EXTRA_FUNCTIONS, abi.PROJ_FUNCTIONS, abi.AST_NGRAM_FUNCTIONS, abi.NAT_NGRAM_FUNCTIONS, abi.CTC_TIMES_FUNCTIONS,
              abi.SCORE_FUNCTIONS, abi.CTC_BIAS_FUNCTIONS, abi.AST_BIAS_FUNCTIONS, abi.FEATS_FUNCTIONS]
    assert sorted(abi.CTC_MERGE_FUNCTIONS) == sorted(NEW) and not any(set(NEW) & set(t) for t in tables)
    with open(abi.CTC_MERGE_HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    found = re.findall(r"^([\w \*]+?)\s*\b(cn_\w+)\s*\(([^()]*)\)\s*;", text, re.M)
    assert sorted(name for _, name, _ in found) == sorted(NEW)
    for flavour in (None, "f16"):
        L = hip.lib(flavour)
        for ret, name, params in found:
            fn = getattr(L, name)
            assert ret.strip() == "int" and fn.restype is C.c_int, name
            assert len(fn.argtypes) == params.count(",") + 1 == len(abi.CTC_MERGE_FUNCTIONS[name][1]), name
            at = 1 if name == "cn_ctc_beam_merged" else 0
            assert list(fn.argtypes[at:at + 3]) == [C.POINTER(hip.CnNgramDesc), C.c_double, C.POINTER(hip.CnBiasDesc)], name
    # the stateless entry and the host entry: cn_op_ctc_bias_beam's arguments behind the two descriptors and lm_scale
    bias = list(abi.CTC_BIAS_FUNCTIONS["cn_op_ctc_bias_beam"][1])[1:]
    assert list(abi.CTC_MERGE_FUNCTIONS["cn_op_ctc_merged_beam"][1])[3:] == bias
    assert list(abi.CTC_MERGE_FUNCTIONS["cn_ctc_merged_beam_host"][1])[3:] == bias[:-1]


@pytest.mark.parametrize("policy", cases.POLICIES)
@pytest.mark.parametrize("beam,pruning", cases.BEAMS)
@pytest.mark.parametrize("Tp", cases.SHAPES)
def test_host_search_is_the_model(Tp, beam, pruning, policy):
    case = cases.make_case(Tp, beam, pruning)
    got, want = cases.run_host(case, policy), cases.model_beams(case, policy)
    cases.same_beams(got, want)
    # the utterance whose every frame is blank (skipped): the empty hypothesis
    assert [e["hyp"] for e in got[2]] == [[]] and got[2][0]["score_ctc"] == 0.0
    # the one cut short saw frames 0 .. int(0.55 * T') only
    assert all(len(e["hyp"]) <= int(np.float32(0.55) * np.float32(Tp)) + 1 for e in got[1])
    for seqs in got:
        assert len({tuple(e["hyp"]) for e in seqs}) == len(seqs)  # the invariant
    if pruning * beam >= 32 * 32:
        assert beam * (case.P + 1) > 256


@pytest.mark.parametrize("policy", cases.POLICIES)
@pytest.mark.parametrize("name", cases.CRAFTED)
def test_host_search_on_the_crafted_cases(name, policy):
    case = cases.crafted(name)
    got = cases.run_host(case, policy)
    cases.same_beams(got, cases.model_beams(case, policy))
    for seqs in got:
        assert len({tuple(e["hyp"]) for e in seqs}) == len(seqs)
    if policy != "none" and name.startswith("abc40"):
        assert any(e["score_lm"] != 0.0 for seqs in got for e in seqs)


def test_the_f16_library_exports_the_same_search():
    case = cases.crafted("abc_lp")
    for policy in cases.POLICIES:
        cases.same_beams(cases.run_host(case, policy, flavour="f16"), cases.run_host(case, policy), tol=0.0)


def test_merging_decides_something():
    """The unmerged host search of the same policy keeps duplicates and, on some utterance, another best hypothesis or score."""
    case = cases.crafted("abc40")
    merged = cases.run_host(case, "bias")
    plain = ctc_bias_cases.run_host(SimpleNamespace(name=cases.PHRASES, **vars(case)))
    assert any(len({tuple(e["hyp"]) for e in seqs}) < len(seqs) for seqs in plain)
    # a sequence both beams hold has, merged, the mass of the paths that the unmerged search spreads over its copies
    gains = [e["score_ctc"] - max(x["score_ctc"] for x in p if x["hyp"] == e["hyp"]) for m, p in zip(merged, plain) for e in m
             if any(x["hyp"] == e["hyp"] for x in p)]
    assert gains and max(gains) > 1e-3


@pytest.mark.parametrize("policy", cases.POLICIES)
@pytest.mark.parametrize("W,P", [(1, 0), (1, 3), (3, 0)])
def test_nothing_to_fold_is_the_unmerged_host_search_bit_for_bit(W, P, policy):
    case = cases.alphabet_case(12, W, P, seed=3)
    got = cases.run_host(case, policy)
    if policy == "ngram":
        want = ctc_ngram_cases.run_host(SimpleNamespace(lm_scale=cases.LM_SCALE, order=cases.ORDER, hash_bits=64, **vars(case)))
    else:
        want = ctc_bias_cases.run_host(SimpleNamespace(name=cases.PHRASES if policy == "bias" else "none", **vars(case)))
    cases.same_beams(got, want, tol=0.0)


@pytest.mark.parametrize("name", ["abc40", "relink", "duplicate"])
def test_no_fusion_in_disguise_is_the_lm_free_search_bit_for_bit(name):
    case = cases.crafted(name)
    want = cases.run_host(case, "none")
    B, Tp, _ = case.logp.shape
    L = hip.lib()
    lm = ctc_ngram_cases.lm_of(cases.ORDER)[0]
    empty = ctc_bias_cases.bias_of("none")
    root = hip.CnBiasDesc()
    root.slots, root.nodes, root.hash_bits = 1, 1, 32
    for ng, scale, bias in ((None, 0.0, empty.desc()), (None, 0.0, root), (lm.desc(), 0.0, None)):
        o = cases.outputs(B, case.W, Tp + 1)
        args, _ = cases.call_args(case, "none", o, Tp + 1)
        args = (C.byref(ng) if ng is not None else None, scale, C.byref(bias) if bias is not None else None) + args[3:]
        assert L.cn_ctc_merged_beam_host(*args) == 0, L.cn_last_error()
        assert cases.untouched(o, B, case.W, Tp + 1)
        got = cases.beams_of(o, B, case.W, Tp + 1)
        if ng is None:
            cases.same_beams(got, want, tol=0.0)
        else:  # (</s> and the open words are scored and multiplied by 0: the order may differ only where keys tie)
            cases.same_beams(got, want, lm_exact=False, lm_bound=0.0, tol=0.0)


def test_refusals_before_any_work():
    L = hip.lib()
    case = cases.make_case(12, 5, 8)
    B, Tp, V = case.logp.shape
    o = cases.outputs(B, 5, Tp + 1, pad=0)
    good = ctc_bias_cases.bias_of(cases.PHRASES).desc()
    lm = ctc_ngram_cases.lm_of(cases.ORDER)[0].desc()

    def edited(**kw):
        d = hip.CnBiasDesc()
        C.memmove(C.byref(d), C.byref(good), C.sizeof(d))
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(fn=L.cn_ctc_merged_beam_host, ng=None, scale=0.0, bias=None, logp=_ptr(case.logp), top=_ptr(case.top), ratio=_ptr(case.ratio), B=B,
             Tp=Tp, V=V, W=5, P=8, lp=0.0, blank=0, hyp=_ptr(o.hyp), cap=Tp + 1, hlen=_ptr(o.hlen), slm=_ptr(o.slm), nb=_ptr(o.nb), tail=()):
        rc = fn(C.byref(ng) if ng is not None else None, scale, C.byref(bias) if bias is not None else None, logp, top, ratio, B, Tp, V, W, P,
                lp, blank, hyp, cap, hlen, _ptr(o.sc), slm, _ptr(o.pb), _ptr(o.pnb), nb, *tail)
        return rc, L.cn_last_error()

    refusals = ((dict(ng=lm, bias=good), b"at most one"), (dict(logp=None), b"null"), (dict(top=None), b"null"), (dict(ratio=None), b"null"),
                (dict(hyp=None), b"null"), (dict(hlen=None), b"null"), (dict(nb=None), b"null"), (dict(slm=None), b"null"),
                (dict(W=0), b"ctc_beam"), (dict(W=33), b"ctc_beam"), (dict(P=-1), b"ctc_pruning"), (dict(P=33), b"ctc_pruning"),
                (dict(bias=edited(slots=good.slots - 1)), b"power of two"), (dict(bias=edited(nodes=-1)), b"negative"),
                (dict(bias=edited(hash_bits=33)), b"hash_bits"), (dict(bias=edited(fail=None)), b"null table"),
                (dict(B=0), b"positive"), (dict(Tp=0), b"positive"), (dict(V=0), b"positive"), (dict(blank=-1), b"blank"), (dict(blank=V), b"blank"),
                (dict(cap=Tp), b"hyp_cap"), (dict(lp=float("nan")), b"number"), (dict(ng=lm, scale=float("nan")), b"number"),
                (dict(ng=lm, W=33), b"ctc_beam"), (dict(bias=good, cap=Tp), b"hyp_cap"))
    for kw, msg in refusals:
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
        # the device entry refuses the same arguments before it touches the GPU
        rc, err = call(fn=L.cn_op_ctc_merged_beam, tail=(None,), **kw)
        assert rc != 0 and msg in err and b"cn_op_ctc_merged_beam" in err, (kw, rc, err)
    for a, s in ((o.hyp, cases.SENT_I), (o.hlen, cases.SENT_I), (o.nb, cases.SENT_I), (o.sc, cases.SENT_F), (o.slm, cases.SENT_F),
                 (o.pb, cases.SENT_F), (o.pnb, cases.SENT_F)):
        assert (a == s).all()
    for kw in (dict(), dict(ng=lm, scale=0.5), dict(bias=good)):
        assert call(**kw)[0] == 0 and (o.nb[:B] >= 1).all()
    assert L.cn_ctc_beam_merged(None, None, 0.0, C.byref(good), None, None, 2, 61, 80, None, 5, 8, 0.2, None, 17, None, None, None, None, None,
                                None, None) != 0
    assert L.cn_last_error()


# ---- ctc_beam_decode, the tasks and the parser ----------------------------------------------------------------------------------------
def test_merging_with_a_fused_transformer_lm_is_refused_before_any_device_call():
    lm = SimpleNamespace(step_engine=lambda n: None)
    for kw, args in ((dict(merge=1), SimpleNamespace(ctc_lm_weight=0.3)), (dict(), SimpleNamespace(ctc_lm_weight=0.3, hip_ctc_merge=1))):
        with pytest.raises(NotImplementedError, match="hip_ctc_merge.*TransformerLM"):
            ctc_beam_decode(None, None, None, None, None, args, lm, **kw)  # (model, features and vocabulary are None: nothing was touched)


@pytest.mark.parametrize("task,decode_type,extra,names", [("cassnat", "att_only", dict(), "att_only"), ("cassnat", "att_only", dict(sample_num=4), "ESA"),
                                                          ("cassnat", "att_only", dict(hip_pipelines=2), "att_only"),
                                                          ("art", "ctc_att", dict(), "ctc_att"), ("art", "ctc_correct", dict(), "ctc_correct")])
def test_tasks_refuse_the_flag_on_paths_without_the_search(task, decode_type, extra, names):
    from cassnat_asr_public_amd.tasks import ArtTask, CassNATTask

    cls = CassNATTask if task == "cassnat" else ArtTask
    self = cls.__new__(cls)  # (decode looks at the arguments before it touches the loader or the model)
    self.test_loader = []
    args = SimpleNamespace(decode_type=decode_type, hip_ctc_merge=1, beam_width=1, **extra)
    with pytest.raises(NotImplementedError, match="hip_ctc_merge") as e:
        cls.decode(self, args)
    assert names in str(e.value)


def test_the_parser_knows_the_flag():
    from cassnat_asr_public_amd.utils.parser import DecodeParser

    base = ["--task", "cassnat", "--test_config", "c.yaml", "--data_path", "f.scp", "--resume_model", "m.mdl", "--result_file", "r.txt"]
    assert DecodeParser().get_args(base).hip_ctc_merge == 0
    assert DecodeParser().get_args(base + ["--hip_ctc_merge", "1"]).hip_ctc_merge == 1
    assert DecodeParser().get_args(base + ["--hip_ctc_merge", "0"]).hip_ctc_merge == 0
    with pytest.raises(SystemExit):
        DecodeParser().get_args(base + ["--hip_ctc_merge", "2"])
