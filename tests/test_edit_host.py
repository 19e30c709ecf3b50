"""The scorer's edit alignment, the parts that need no GPU: the companion header and its binding, the host entry cn_edit_align_host in
both libraries against the model (tests/edit_model.py) on the whole case list, every output byte and every sentinel, the refusals of
both entry points, and the host side (utils/score.py, bin/score_asr --host) on hand-written strings."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest

import edit_cases
from cassnat_asr_public_amd import abi, hip
from cassnat_asr_public_amd.utils import score
from cassnat_asr_public_amd.utils.parser import DecodeParser

NEW = ["cn_op_edit_align", "cn_edit_align_host"]
SEP = "▁"


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_call(L):
    def call(a):
        return L.cn_edit_align_host(p(a["ref"]), a["ref_total"], p(a["ref_begin"]), p(a["ref_len"]), p(a["hyp"]), a["hyp_total"], p(a["hyp_begin"]),
                                    p(a["hyp_len"]), a["N"], a["max_ref"], a["max_hyp"], *a["costs"], p(a["cost"]), p(a["counts"]), p(a["path_len"]),
                                    p(a["ops"]), a["ops_total"], p(a["ops_begin"]))
    return call


def test_entry_points_are_declared_in_the_new_header_only_and_exported_by_both_libraries():
    assert sorted(abi.SCORE_FUNCTIONS) == sorted(NEW)
    older = (set(abi.FUNCTIONS) | set(abi.EXTRA_FUNCTIONS) | set(abi.PROJ_FUNCTIONS) | set(abi.AST_NGRAM_FUNCTIONS) | set(abi.NAT_NGRAM_FUNCTIONS)
             | set(abi.CTC_TIMES_FUNCTIONS))
    assert not set(NEW) & older
    with open(abi.SCORE_HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    assert "struct" not in text                                            # plain arguments only
    found = re.findall(r"^([\w \*]+?)\s*\b(cn_\w+)\s*\(([^()]*)\)\s*;", text, re.M)
    assert sorted(name for _, name, _ in found) == sorted(NEW)
    for flavour in (None, "f16"):
        L = hip.lib(flavour)
        for ret, name, params in found:
            fn = getattr(L, name)
            assert ret.strip() == "int" and fn.restype is C.c_int, name
            assert len(fn.argtypes) == params.count(",") + 1 == len(abi.SCORE_FUNCTIONS[name][1]), name
    assert [len(abi.SCORE_FUNCTIONS[n][1]) for n in NEW] == [22, 20]
    # the older headers keep their lists
    assert len(abi.FUNCTIONS) == 121 and len(hip.declared_symbols()) == 121 and len(abi.CTC_TIMES_FUNCTIONS) == 3


@pytest.mark.parametrize("flavour", [None, "f16"])
@pytest.mark.parametrize("name", [c["name"] for c in edit_cases.cases()])
def test_host_entry_is_the_model_in_every_byte(name, flavour):
    assert edit_cases.run_entry(edit_cases.by_name(name), host_call(hip.lib(flavour))) == []


def test_python_entry_on_numpy_arrays():
    case = edit_cases.by_name("n70-shared-433")
    cost, counts, plen, ops, ob = hip.edit_align_host(case["ref"], case["ref_begin"], case["ref_len"], case["hyp"], case["hyp_begin"], case["hyp_len"],
                                                      case["costs"])
    w_cost, w_counts, w_plen, w_paths = edit_cases._expected(case["name"])
    assert cost.tolist() == w_cost and counts.tolist() == w_counts and plen.tolist() == w_plen
    assert [ops[b:b + n].tolist() for b, n in zip(ob, plen)] == w_paths


def test_refusals_before_anything_runs():
    """A null buffer, N, max_ref, max_hyp or a cost out of range, a negative total: the host entry and - the same check in front of its
    launch, which is never reached - the device entry."""
    L = hip.lib()
    case = edit_cases.by_name("n3-111")
    names = ("ref", "ref_begin", "ref_len", "hyp", "hyp_begin", "hyp_len", "ops_begin", "cost", "counts", "path_len", "ops")

    def refused(device, **kw):
        kept = {}

        def call(a):
            kept.update(a)
            b = dict(a, **{k: v for k, v in kw.items() if k not in ("tri_at", "tri")})
            if "tri_at" in kw:
                costs = list(b["costs"])
                costs[kw["tri_at"]] = kw["tri"]
                b["costs"] = tuple(costs)
            if not device:
                return host_call(L)(b)
            return L.cn_op_edit_align(p(b["ref"]), b["ref_total"], p(b["ref_begin"]), p(b["ref_len"]), p(b["hyp"]), b["hyp_total"], p(b["hyp_begin"]),
                                      p(b["hyp_len"]), b["N"], b["max_ref"], b["max_hyp"], *b["costs"], -1, p(b["cost"]), p(b["counts"]), p(b["path_len"]),
                                      p(b["ops"]), b["ops_total"], p(b["ops_begin"]), None)
        got = edit_cases.run_entry(case, call)
        untouched = ((kept["cost"] == edit_cases.SENT_I).all() and (kept["counts"] == edit_cases.SENT_I).all()
                     and (kept["path_len"] == edit_cases.SENT_I).all() and (kept["ops"] == edit_cases.SENTINEL).all())
        return got[0] == "rc -1" and untouched, L.cn_last_error().decode()   # (refused, and nothing was written)

    bad = [({k: None}, "null argument") for k in names]
    bad += [(dict(N=0), "N must"), (dict(N=(1 << 20) + 1), "N must"), (dict(max_ref=-1), "max_ref must"), (dict(max_ref=8193), "max_ref must"),
            (dict(max_hyp=-1), "max_hyp must"), (dict(max_hyp=8193), "max_hyp must"), (dict(ref_total=-1), "sizes"), (dict(ops_total=-5), "sizes")]
    bad += [(dict(tri_at=k, tri=c), "costs must") for k in range(3) for c in (0, 256, -1)]
    for device in (False, True):
        for kw, what in bad:
            ok, msg = refused(device, **kw)
            assert ok and what in msg and ("cn_op_edit_align" if device else "cn_edit_align_host") in msg, (device, kw, msg)


# ---- utils/score.py on hand-written strings ---------------------------------------------------------------------------------------------
def vocab_of(pieces):
    return SimpleNamespace(index2word=dict(enumerate(["blank", "sos", "eos", "unk"] + pieces)))


REF = {"u1": [SEP + "the", SEP + "c", "at", SEP + "sat"], "u2": [SEP + "on", SEP + "the", SEP + "m", "at"], "u3": [SEP + "a", SEP + "b"],
       "u4": [SEP + "gone"]}
HYP = {"u1": [SEP + "the", SEP + "c", "at", SEP + "sat"], "u2": [SEP + "on", SEP + "m", "at"], "u3": [SEP + "b", SEP + "b", SEP + "c"]}
ORDER = ["u1", "u2", "u3"]
REF_ORDER = ["u1", "u2", "u3", "u4"]


def test_units_from_pieces_words_and_chars():
    pieces = [SEP + "the", SEP + "c", "at", SEP, SEP + "sat"]
    assert score.to_units(pieces, "pieces", "word") == ["the", "cat", "sat"]
    assert score.to_units(pieces, "pieces", "token") == pieces
    assert score.to_units(pieces, "pieces", "char") == list("thecatsat")
    assert score.to_units(["the", "cat"], "words", "word") == ["the", "cat"]
    assert score.to_units(["the", "cat"], "words", "char") == list("thecat")
    assert score.to_units([], "pieces", "word") == [] and score.to_units([], "words", "char") == []
    with pytest.raises(score.ScoreError, match="pieces"):
        score.to_units(["the"], "words", "token")
    # a vocabulary without separator pieces is scored per token; char stays char
    assert score.unit_of("word", vocab_of(["a", "b"])) == "token" and score.unit_of("word", vocab_of([SEP + "a", "b"])) == "word"
    assert score.unit_of("char", vocab_of(["a", "b"])) == "char" and score.unit_of("word", None) == "word"
    assert score.parse_costs("4,3,3") == (4, 3, 3)
    for bad in ("1,1", "0,1,1", "1,256,1", "a,b,c"):
        with pytest.raises(score.ScoreError, match="hip_score_costs"):
            score.parse_costs(bad)


WER_PRESENT = """%WER 37.50 [ 3 / 8, 1 ins, 1 del, 1 sub ]
%SER 66.67 [ 2 / 3 ]
Scored 3 sentences, 1 not present in hyp.
unit word, costs sub 1 ins 1 del 1
"""
PER_UTT_PRESENT = """u1 ref the cat sat
u1 hyp the cat sat
u1 op C C C
u1 #csid 3 0 0 0
u2 ref on the mat
u2 hyp on *** mat
u2 op C D C
u2 #csid 2 0 0 1
u3 ref a b ***
u3 hyp b b c
u3 op S C I
u3 #csid 1 1 1 0
"""
WER_ALL = """%WER 44.44 [ 4 / 9, 1 ins, 2 del, 1 sub ]
%SER 75.00 [ 3 / 4 ]
Scored 4 sentences, 1 not present in hyp.
unit word, costs sub 1 ins 1 del 1
"""
PER_UTT_U4 = """u4 ref gone
u4 hyp ***
u4 op D
u4 #csid 0 0 0 1
"""


def write_table(path, order, table):
    path.write_text("".join(" ".join([u] + table[u]) + "\n" for u in order), encoding="utf-8")
    return str(path)


def read(path):
    return open(path, encoding="utf-8").read()


def test_score_files_byte_for_byte(tmp_path):
    """Worked by hand from the definition.  u2: the / on must go (D).  u3, a b against b b c, from the end: c is cheapest as an insertion (I),
    b is b (C), a becomes b (S)."""
    res = score.score(ORDER, HYP, REF_ORDER, REF, host=True)
    res.write(str(tmp_path / "present"))
    assert read(tmp_path / "present" / "wer") == WER_PRESENT
    assert read(tmp_path / "present" / "per_utt") == PER_UTT_PRESENT
    assert read(tmp_path / "present" / "ref.trn") == "the cat sat (u1)\non the mat (u2)\na b (u3)\n"
    assert read(tmp_path / "present" / "hyp.trn") == "the cat sat (u1)\non mat (u2)\nb b c (u3)\n"
    res = score.score(ORDER, HYP, REF_ORDER, REF, mode="all", host=True)
    res.write(str(tmp_path / "all"))
    assert read(tmp_path / "all" / "wer") == WER_ALL
    assert read(tmp_path / "all" / "per_utt") == PER_UTT_PRESENT + PER_UTT_U4
    assert read(tmp_path / "all" / "hyp.trn").endswith("b b c (u3)\n(u4)\n")
    # tokens and characters, other costs; words against a reference in words
    tok = score.score(ORDER, HYP, REF_ORDER, REF, unit="token", costs=(4, 3, 3), host=True)
    assert tok.wer_lines()[0] == "%WER 30.00 [ 3 / 10, 1 ins, 1 del, 1 sub ]" and tok.wer_lines()[3] == "unit token, costs sub 4 ins 3 del 3"
    ch = score.score(ORDER, HYP, REF_ORDER, REF, unit="char", host=True)
    assert ch.per_utt_lines("u2") == ["u2 ref o n t h e m a t", "u2 hyp o n *** *** *** m a t", "u2 op C C D D D C C C", "u2 #csid 5 0 0 3"]
    words = {u: score.to_units(REF[u], "pieces", "word") for u in REF}
    assert score.score(ORDER, HYP, REF_ORDER, words, ref_form="words", host=True).wer_lines() == WER_PRESENT.splitlines()


def test_score_error_cases():
    with pytest.raises(score.ScoreError, match="u9 of the hypothesis file has no reference"):
        score.score(ORDER + ["u9"], dict(HYP, u9=["x"]), REF_ORDER, REF, host=True)
    with pytest.raises(score.ScoreError, match="no unit at all"):
        score.score(["u1"], {"u1": [SEP + "a"]}, ["u1"], {"u1": []}, host=True)
    with pytest.raises(score.ScoreError, match="no unit at all"):
        score.score(["u1"], {"u1": [SEP + "a"]}, ["u1"], {"u1": [SEP]}, host=True)
    with pytest.raises(score.ScoreError, match="needs a reference in pieces"):
        score.score(ORDER, HYP, REF_ORDER, REF, unit="token", ref_form="words", host=True)
    with pytest.raises(score.ScoreError, match="neither present nor all"):
        score.score(ORDER, HYP, REF_ORDER, REF, mode="some", host=True)
    with pytest.raises(score.ScoreError, match="more than 8192 units"):
        score.score(["u1"], {"u1": ["a"] * 8193}, ["u1"], {"u1": ["a"]}, unit="token", host=True)
    with pytest.raises(score.ScoreError, match="needs references"):
        score.score_run(SimpleNamespace(hip_score="x", text_label=""), None, ORDER, HYP)


def test_score_run_reads_text_label_by_default(tmp_path, capsys):
    ref = write_table(tmp_path / "token.scp", REF_ORDER, REF)
    other = write_table(tmp_path / "other.scp", REF_ORDER, dict(REF, u2=HYP["u2"]))
    args = SimpleNamespace(hip_score=str(tmp_path / "a"), text_label=ref, hip_score_ref="", hip_score_unit="word", hip_score_ref_form="pieces",
                           hip_score_costs="1,1,1", hip_score_mode="present")
    vocab = vocab_of(sorted({x for v in REF.values() for x in v}))
    assert score.score_run(args, vocab, ORDER, HYP, host=True) == WER_PRESENT.splitlines()[0] == capsys.readouterr().out.strip()
    assert read(tmp_path / "a" / "per_utt") == PER_UTT_PRESENT
    args.hip_score_ref, args.hip_score = other, str(tmp_path / "b")
    assert score.score_run(args, vocab, ORDER, HYP, host=True) == "%WER 28.57 [ 2 / 7, 1 ins, 0 del, 1 sub ]"


def test_many_pairs_go_through_in_bounded_calls(monkeypatch):
    """The run is split only to bound the aligner's scratch: the same result from one call and from many."""
    import random

    rng = random.Random(5)
    order = ["u%03d" % k for k in range(40)]
    refs = {u: ["w%d" % rng.randrange(6) for _ in range(rng.randrange(0, 30))] for u in order}
    refs["u000"] = ["w1"]
    hyps = {u: [w for w in refs[u] if rng.random() > 0.2] + ["w%d" % rng.randrange(6)] * rng.randrange(0, 3) for u in order}
    one = score.score(order, hyps, order, refs, unit="token", host=True)
    monkeypatch.setattr(score, "SCRATCH_BOUND", 4096)
    many = score.score(order, hyps, order, refs, unit="token", host=True)
    assert one.wer_lines() == many.wer_lines() and one.path == many.path and one.counts == many.counts


def test_flags_are_parsed():
    a = DecodeParser().get_args(["--hip_score", "d", "--hip_score_unit", "char", "--hip_score_ref", "r", "--hip_score_ref_form", "words",
                                 "--hip_score_costs", "4,3,3", "--hip_score_mode", "all"])
    assert (a.hip_score, a.hip_score_unit, a.hip_score_ref, a.hip_score_ref_form, a.hip_score_costs, a.hip_score_mode) == ("d", "char", "r", "words", "4,3,3", "all")
    d = DecodeParser().get_args([])
    assert (d.hip_score, d.hip_score_unit, d.hip_score_ref, d.hip_score_ref_form, d.hip_score_costs, d.hip_score_mode) == ("", "word", "", "pieces", "1,1,1", "present")


def test_score_asr_host_writes_exactly_those_files(tmp_path, capsys):
    from cassnat_asr_public_amd.bin import score_asr

    hyp, ref = write_table(tmp_path / "result.txt", ORDER, HYP), write_table(tmp_path / "token.scp", REF_ORDER, REF)
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("".join(x + "\n" for x in sorted({x for v in list(REF.values()) + list(HYP.values()) for x in v})), encoding="utf-8")
    out = tmp_path / "score"
    assert score_asr.main(["--hyp", hyp, "--ref", ref, "--vocab_file", str(vocab), "--out", str(out), "--host"]) == 0
    assert "%WER 37.50 [ 3 / 8, 1 ins, 1 del, 1 sub ]" in capsys.readouterr().out
    assert sorted(x.name for x in out.iterdir()) == ["hyp.trn", "per_utt", "ref.trn", "wer"]
    assert read(out / "wer") == WER_PRESENT and read(out / "per_utt") == PER_UTT_PRESENT
    out_all = tmp_path / "score_all"
    assert score_asr.main(["--hyp", hyp, "--ref", ref, "--vocab_file", str(vocab), "--out", str(out_all), "--host", "--hip_score_mode", "all"]) == 0
    assert read(out_all / "wer") == WER_ALL
    # an utterance without a reference: exit status 1 and its name
    bad = write_table(tmp_path / "bad.txt", ["u1", "zz"], {"u1": HYP["u1"], "zz": [SEP + "a"]})
    assert score_asr.main(["--hyp", bad, "--ref", ref, "--out", str(tmp_path / "bad"), "--host"]) == 1
    assert "zz" in capsys.readouterr().err
