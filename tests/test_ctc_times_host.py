"""CTC token time stamps, the parts that need no GPU: the companion header and its binding, the refusals of the entry points, the
host entry cn_ctc_token_times_host against the numpy model (tests/ctc_times_model.py) bit for bit on the whole case list, and the
file-writing side (utils/ctm.py) on hand-written spans."""
import ctypes as C
import math
import re
from types import SimpleNamespace

import numpy as np
import pytest

import ctc_times_cases as cases
from cassnat_asr_public_amd import abi, hip
from cassnat_asr_public_amd.utils import ctm
from cassnat_asr_public_amd.utils.parser import DecodeParser


def test_entry_points_are_declared_in_the_new_header_only_and_exported_by_both_libraries():
    assert sorted(abi.CTC_TIMES_FUNCTIONS) == sorted(cases.NEW)
    assert not set(cases.NEW) & (set(abi.FUNCTIONS) | set(abi.EXTRA_FUNCTIONS) | set(abi.PROJ_FUNCTIONS) | set(abi.AST_NGRAM_FUNCTIONS)
                                 | set(abi.NAT_NGRAM_FUNCTIONS))
    with open(abi.CTC_TIMES_HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    found = re.findall(r"^([\w \*]+?)\s*\b(cn_\w+)\s*\(([^()]*)\)\s*;", text, re.M)
    assert sorted(name for _, name, _ in found) == sorted(cases.NEW)
    for flavour in (None, "f16"):
        L = hip.lib(flavour)
        for ret, name, params in found:
            fn = getattr(L, name)
            assert ret.strip() == "int" and fn.restype is C.c_int, name
            assert len(fn.argtypes) == params.count(",") + 1 == len(abi.CTC_TIMES_FUNCTIONS[name][1]), name
    assert [len(abi.CTC_TIMES_FUNCTIONS[n][1]) for n in cases.NEW] == [16, 15, 16]
    # the older headers keep their lists, the option structs their sizes
    assert len(abi.FUNCTIONS) == 121 and len(abi.EXTRA_FUNCTIONS) == 3 and len(abi.AST_NGRAM_FUNCTIONS) == 6 and len(abi.NAT_NGRAM_FUNCTIONS) == 5
    assert C.sizeof(hip.CnDecodeOpts) == 64 and C.sizeof(hip.CnAstOpts) == 56


@pytest.mark.parametrize("flavour", [None, "f16"])
@pytest.mark.parametrize("name", [c.name for c in cases.cases()])
def test_host_entry_is_the_model_bit_for_bit(name, flavour):
    c = cases.case(name)
    cases.same_as_model(c, cases.run_host(c, hip.lib(flavour)))


def test_refusals_before_anything_runs():
    """A null buffer and B, T', V, ld or the blank out of range: the host entry and - the same check in front of its launch, which is
    never reached - the device entry; the model entry refuses a null handle."""
    L = hip.lib()
    c = cases.case("t7_soft")
    B, Tp, V = c.logp.shape
    ld = c.labels.shape[1]
    bufs = dict(zip(("start", "end", "conf", "score", "status"), cases.out_buffers(c)))
    ins = dict(logp=c.logp, frames=c.frames, labels=c.labels, label_len=c.label_len)

    def call(fn, extra=(), **kw):
        a = dict(ins, **bufs)
        n = dict(B=B, Tp=Tp, V=V, ld=ld, blank=c.blank)
        for k, v in kw.items():
            (a if k in a else n)[k] = v
        q = {k: (cases.p(v) if v is not None else None) for k, v in a.items()}
        return fn(q["logp"], q["frames"], q["labels"], n["ld"], q["label_len"], n["B"], n["Tp"], n["V"], n["blank"], -1, q["start"], q["end"],
                  q["conf"], q["score"], q["status"], *extra)

    bad = [(dict([(k, None)]), "null argument") for k in list(ins) + list(bufs)]
    bad += [(dict(B=0), "B must"), (dict(B=(1 << 16) + 1), "B must"), (dict(Tp=0), "T' must"), (dict(Tp=(1 << 16) + 1), "T' must"),
            (dict(V=0), "V must"), (dict(V=(1 << 20) + 1), "V must"), (dict(ld=0), "ld must"), (dict(ld=1501), "ld must"), (dict(ld=-3), "ld must"),
            (dict(blank=-1), "blank"), (dict(blank=V), "blank")]
    for fn, extra in ((L.cn_ctc_token_times_host, ()), (L.cn_op_ctc_token_times, (None,))):
        for kw, what in bad:
            assert call(fn, extra, **kw) == -1 and what in L.cn_last_error().decode(), (kw, L.cn_last_error())
    assert all((b == s).all() for b, s in zip(bufs.values(), cases.out_buffers(c)))  # a refused call wrote nothing
    assert call(L.cn_ctc_token_times_host) == 0                                      # and the same call with nothing wrong runs
    cases.same_as_model(c, tuple(bufs.values()))
    assert L.cn_ctc_token_times(None, None, None, 1, 16, 80, None, None, 4, None, None, None, None, None, None, None) != 0


# ---- utils/ctm.py on hand-written spans ----------------------------------------------------------------------------------------------
SEC = 0.04
LP = [math.log(0.9), math.log(0.5), math.log(0.8), math.log(0.25)]


def test_pieces_merge_into_words():
    rec = (["▁he", "llo", "▁wor", "ld"], [2, 5, 9, 12], [4, 8, 11, 20], LP, 0, 30)
    assert ctm.units(rec[0], "word") == [(0, 1, "hello"), (2, 3, "world")]
    assert ctm.lines("utt1", rec, SEC, "word") == ["utt1 1 0.08 0.24 hello 0.500", "utt1 1 0.36 0.44 world 0.250"]
    # a hypothesis that begins inside a word: the first piece starts a word all the same
    assert ctm.units(["llo", "▁x"], "word") == [(0, 0, "llo"), (1, 1, "x")]
    # separators alone are no word; doubled separators vanish as in the detokenised line
    assert ctm.units(["▁", "▁▁a", "▁", "b"], "word") == [(1, 1, "a"), (2, 3, "b")]


def test_token_mode_and_a_vocabulary_without_separators():
    rec = (["▁he", "llo"], [2, 5], [4, 8], LP[:2], 0, 30)
    assert ctm.lines("u", rec, SEC, "token") == ["u 1 0.08 0.08 ▁he 0.900", "u 1 0.20 0.12 llo 0.500"]
    with_sep = SimpleNamespace(index2word={0: "blank", 4: "▁a", 5: "b"})
    without = SimpleNamespace(index2word={0: "blank", 4: "w0", 5: "w1"})
    assert ctm.unit_of(SimpleNamespace(hip_ctm_unit="word"), with_sep) == "word"
    assert ctm.unit_of(SimpleNamespace(hip_ctm_unit="token"), with_sep) == "token"
    assert ctm.unit_of(SimpleNamespace(hip_ctm_unit="word"), without) == "token"
    assert ctm.unit_of(SimpleNamespace(), with_sep) == "word"
    rec = (["w0", "w1"], [0, 3], [3, 4], LP[:2], 0, 9)
    assert ctm.lines("u", rec, SEC, ctm.unit_of(SimpleNamespace(), without)) == ["u 1 0.00 0.12 w0 0.900", "u 1 0.12 0.04 w1 0.500"]


def test_an_unaligned_utterance_spreads_its_units_evenly_and_an_empty_one_writes_nothing(tmp_path):
    bad = (["▁a", "b", "▁c", "▁d"], [-1] * 4, [-1] * 4, [0.0] * 4, 1, 30)            # status 1: three words over 30 frames
    assert ctm.lines("u", bad, SEC, "word") == ["u 1 0.00 0.40 ab 0.000", "u 1 0.40 0.40 c 0.000", "u 1 0.80 0.40 d 0.000"]
    hole = (["▁a", "▁b"], [0, -1], [4, -1], [LP[0], 0.0], 0, 10)                     # a label the walk never entered
    assert ctm.lines("u", hole, SEC, "word") == ["u 1 0.00 0.20 a 0.000", "u 1 0.20 0.20 b 0.000"]
    empty = ([], [], [], [], 0, 12)
    assert ctm.lines("u", empty, SEC, "word") == []
    good = (["▁a"], [1], [3], [LP[2]], 0, 10)
    path = tmp_path / "out.ctm"
    missed = ctm.write(str(path), ["u2", "u0", "u1", "u3"], {"u0": bad, "u1": empty, "u2": good, "u3": hole}, SEC, "word")
    assert missed == 2
    assert path.read_text(encoding="utf-8").splitlines() == ["u2 1 0.04 0.08 a 0.800"] + ctm.lines("u0", bad, SEC, "word") + ctm.lines("u3", hole, SEC, "word")


def test_timing_labels_and_flags():
    assert ctm.seconds_per_frame(SimpleNamespace(skip_frame=1)) == pytest.approx(0.04)
    assert ctm.seconds_per_frame(SimpleNamespace(skip_frame=3, hip_fbank_conf="")) == pytest.approx(0.12)
    vocab = SimpleNamespace(word2index={"blank": 0, "sos": 1, "eos": 2, "unk": 3})
    assert ctm.label_ids([1, 7, 0, 3, 9, 2, 8], vocab, 0) == [7, 3, 9]
    args = DecodeParser().get_args(["--hip_ctm", "x.ctm", "--hip_ctm_unit", "token"])
    assert args.hip_ctm == "x.ctm" and args.hip_ctm_unit == "token"
    args = DecodeParser().get_args([])
    assert args.hip_ctm == "" and args.hip_ctm_unit == "word"
    with pytest.raises(SystemExit):
        DecodeParser().get_args(["--hip_ctm_unit", "phone"])
    # a confidence is a probability even when a log-posterior rounds above 0
    assert ctm.lines("u", (["a"], [0], [1], [1e-7], 0, 1), SEC, "token") == ["u 1 0.00 0.04 a 1.000"]
