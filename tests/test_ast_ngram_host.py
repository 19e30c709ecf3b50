"""AST beam search with word n-gram fusion, the parts that need no GPU: the companion header and its binding, the host entry
cn_ast_ngram_adds_host against the numpy model (tests/ast_ngram_model.py), the invariant that the terms along a hypothesis sum to
the sentence's ARPA score, and ArtTask.load_lm_model with rank_model n-gram."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest

import ast_ngram_cases as cases
import ast_ngram_model as model_of
from cassnat_asr_public_amd import abi, hip
from cassnat_asr_public_amd.models.ngram import NgramLM
from cassnat_asr_public_amd.tasks.art_task import ArtTask
from ctc_ngram_cases import collision_case
from ctc_ngram_model import raw_of
from ngram_model import random_arpa

LD = 41


def test_entry_points_are_declared_in_the_new_header_only_and_exported_by_both_libraries():
    assert sorted(abi.AST_NGRAM_FUNCTIONS) == sorted(cases.NEW)
    assert not set(cases.NEW) & (set(abi.FUNCTIONS) | set(abi.EXTRA_FUNCTIONS) | set(abi.PROJ_FUNCTIONS))
    with open(abi.AST_NGRAM_HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    found = re.findall(r"^([\w \*]+?)\s*\b(cn_\w+)\s*\(([^()]*)\)\s*;", text, re.M)
    assert sorted(name for _, name, _ in found) == sorted(cases.NEW)
    for flavour in (None, "f16"):
        L = hip.lib(flavour)
        for ret, name, params in found:
            fn = getattr(L, name)
            assert ret.strip() == "int" and fn.restype is C.c_int, name
            assert len(fn.argtypes) == params.count(",") + 1 == len(abi.AST_NGRAM_FUNCTIONS[name][1]), name
    # the two older headers keep their lists, cn_ast_opts its size
    assert len(abi.FUNCTIONS) == 121 and len(abi.EXTRA_FUNCTIONS) == 3 and C.sizeof(hip.CnAstOpts) == 56


@pytest.mark.parametrize("order", cases.ORDERS)
def test_host_adds_are_the_model_bit_for_bit(order):
    lm, model = cases.lm_of(order)
    rows = cases.crafted(LD) + cases.random_rows(np.random.RandomState(order), 40, LD)
    tok, lens = cases.pack(rows, LD)
    got = cases.host_adds(lm, tok, lens)
    cases.same_bits(got, cases.model_adds(model, rows))
    # through the model class
    cases.same_bits(lm.ast_adds_host(tok, lens, cases.EOS), got)
    # an empty hypothesis pays </s> after <s> when it ends, nothing when a word begins
    assert got[0, 0] == 0.0 and got[0, 1] == np.float32(model.word_score(["<s>"], "</s>"))
    # a length beyond the stride is the stride, a negative one the empty row
    lens2 = lens.copy()
    lens2[1], lens2[2] = -4, LD + 9
    got2 = cases.host_adds(lm, tok, lens2)
    want2 = cases.model_adds(model, [rows[0], [], tok[2].tolist()] + rows[3:])
    cases.same_bits(got2, want2)


def test_another_eos_id_is_another_gluing():
    lm, model = cases.lm_of(3)
    rows = [[cases.IX["▁a"], cases.IX["b"], cases.IX["bc"]], [cases.IX["▁a"], cases.EOS, cases.IX["▁c"]]]
    tok, lens = cases.pack(rows, 5)
    for eos in (cases.EOS, cases.IX["b"], -1):
        cases.same_bits(cases.host_adds(lm, tok, lens, eos=eos), cases.model_adds(model, rows, eos=eos))


def test_colliding_word_keys():
    case = collision_case()
    lm, model = cases.lm_of(1, case.hash_bits)
    spell = [[cases.IX["▁zz"]] + [cases.IX[c] for c in w[2:]] if w.startswith("zz") else [cases.IX["▁" + w[0]]] + [cases.IX[c] for c in w[1:]]
             for w in case.hit[:4]]
    rows = spell + [[cases.IX["▁a"]] + s for s in spell] + [s + [cases.IX["▁"]] for s in spell] + cases.crafted(LD)
    tok, lens = cases.pack(rows, LD)
    got = cases.host_adds(lm, tok, lens)
    cases.same_bits(got, cases.model_adds(model, rows))
    _, untold = cases.lm_of(1)
    assert (got.view(np.int32) != cases.model_adds(untold, rows).view(np.int32)).any()  # a word outside the model was taken for one of it


@pytest.mark.parametrize("order", cases.ORDERS)
def test_terms_along_a_hypothesis_sum_to_the_sentence_score(order):
    """What the search adds for a finished hypothesis - the term of every token given the tokens before it, eos last - is the ARPA
    score of its text; exact on a dyadic model."""
    lm, model = cases.lm_of(order)
    starts = model_of.starts_of(cases.VOCAB)
    rng = np.random.RandomState(50 + order)
    seqs = [[t for t in r if 0 <= t < cases.V and t != cases.EOS] for r in cases.random_rows(rng, 25, 24)] + [[]]
    for seq in seqs:
        prefixes = [seq[:i] for i in range(len(seq) + 1)]
        tok, lens = cases.pack(prefixes, max(1, len(seq)))
        adds = cases.host_adds(lm, tok, lens)
        total = np.float32(0.0)
        for i, c in enumerate(seq):
            total = np.float32(total + model_of.term(adds[i], starts, cases.EOS, c))
        total = np.float32(total + model_of.term(adds[len(seq)], starts, cases.EOS, cases.EOS))
        assert float(total) == model.score(raw_of(seq, cases.VOCAB, drop_id=cases.EOS))[0], seq


def test_host_entry_refusals():
    lm, _ = cases.lm_of(3)
    L = hip.lib()
    tok, lens = cases.pack([[4, 5]], 4)
    out = np.zeros(2, np.float32)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def refused(desc, n=1, ld=4, what=""):
        rc = L.cn_ast_ngram_adds_host(C.byref(desc) if desc is not None else None, P(tok), ld, P(lens), n, cases.EOS, P(out))
        assert rc != 0 and what in L.cn_last_error().decode(), L.cn_last_error()

    def changed(**kw):
        d = hip.CnNgramDesc.from_buffer_copy(lm.desc())
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    refused(None, what="null")
    refused(lm.desc(), n=0, what="rows")
    refused(lm.desc(), ld=0, what="stride")
    refused(changed(order=0), what="order 0 is outside 1 .. 8")
    refused(changed(order=9), what="order 9 is outside 1 .. 8")
    refused(changed(gram_slots=48), what="powers of two")
    refused(changed(word_slots=0), what="powers of two")
    refused(changed(piece_starts=None), what="null table")


def _task():
    return SimpleNamespace(vocab=cases.VOCAB, model=SimpleNamespace(_device=0), lm_model=None)


def test_art_task_loads_an_arpa_model_for_rank_model_ngram(tmp_path):
    path = tmp_path / "m.arpa"
    path.write_text(random_arpa(cases.WORDS, 3, seed=4), encoding="utf-8")
    task = _task()
    args = SimpleNamespace(lm_weight=0.5, ctc_lm_weight=0, decode_type="ctc_att", rank_model="n-gram", rnnlm=str(path), lm_config=None)
    ArtTask.load_lm_model(task, args)
    assert isinstance(task.lm_model, NgramLM) and task.lm_model.order == 3 and task.lm_model.vocab_size == cases.V
    assert ArtTask._lm_engines(task, 3, SimpleNamespace(batch_size=2, beam_width=2)) == [None] * 3  # the workers share its tables
    # lm_weight 0: no model is read
    args.lm_weight = 0
    ArtTask.load_lm_model(task, args)
    assert task.lm_model is None


def test_art_task_refuses_a_file_that_is_no_arpa_text(tmp_path):
    path = tmp_path / "m.bin"
    path.write_bytes(b"mmap lm http://kheafield.com/code format version 5\n\0\0\0\0")
    args = SimpleNamespace(lm_weight=0.5, ctc_lm_weight=0, decode_type="ctc_att", rank_model="n-gram", rnnlm=str(path), lm_config=None)
    with pytest.raises(NotImplementedError, match="ARPA"):
        ArtTask.load_lm_model(_task(), args)
    # and outside ctc_att the n-gram model is not fused either
    args.decode_type = "ctc_correct"
    with pytest.raises(NotImplementedError, match="ctc_att"):
        ArtTask.load_lm_model(_task(), args)
