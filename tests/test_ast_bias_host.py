"""AST beam search with contextual phrase biasing, the parts that need no GPU: the companion header and its binding, the host twins
cn_ast_bias_nodes_host / cn_ast_bias_terms_host against the numpy model (tests/ast_bias_model.py) bit for bit, every refusal that is
reached without a GPU call, the parser's --hip_bias_search, the tasks' refusals of `att` on the wrong paths and beam_decode's refusal
of a list beside a fused language model."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest

import ast_bias_cases as cases
import ast_bias_model as model
from cassnat_asr_public_amd import abi, hip
from cassnat_asr_public_amd.models.ngram import _ptr

LD = 41


def test_entry_points_are_declared_in_the_new_header_only_and_exported_by_both_libraries():
    assert sorted(abi.AST_BIAS_FUNCTIONS) == sorted(cases.NEW)
    older = (set(abi.FUNCTIONS) | set(abi.EXTRA_FUNCTIONS) | set(abi.PROJ_FUNCTIONS) | set(abi.AST_NGRAM_FUNCTIONS) | set(abi.NAT_NGRAM_FUNCTIONS)
             | set(abi.CTC_TIMES_FUNCTIONS) | set(abi.SCORE_FUNCTIONS) | set(abi.CTC_BIAS_FUNCTIONS))
    assert not set(cases.NEW) & older
    with open(abi.AST_BIAS_HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    found = re.findall(r"^([\w \*]+?)\s*\b(cn_\w+)\s*\(([^()]*)\)\s*;", text, re.M)
    assert sorted(name for _, name, _ in found) == sorted(cases.NEW)
    assert "typedef" not in text  # cn_bias_desc stays where it is, unchanged
    for flavour in (None, "f16"):
        L = hip.lib(flavour)
        for ret, name, params in found:
            fn = getattr(L, name)
            assert ret.strip() == "int" and fn.restype is C.c_int, name
            assert len(fn.argtypes) == params.count(",") + 1 == len(abi.AST_BIAS_FUNCTIONS[name][1]), name
    assert len(abi.CTC_BIAS_FUNCTIONS) == 3 and C.sizeof(hip.CnBiasDesc) == 64 and C.sizeof(hip.CnAstOpts) == 56
    assert abi.AST_BIAS_FUNCTIONS["cn_ast_attach_bias"][1][1] is C.POINTER(hip.CnBiasDesc)


@pytest.mark.parametrize("name", cases.NINE + ["chain"])
def test_host_twins_are_the_model_bit_for_bit(name):
    """Both host twins on every row of the set - the empty row, planted phrases, ids outside the vocabulary, a row of full length -
    and every candidate id of the vocabulary, one below and two above it, and eos; sentinels behind every output (cases.host_*)."""
    bias = cases.bias_of(name)
    rows = cases.rows_of(name, LD)
    tok, lens = cases.pack(rows, LD)
    nodes = cases.host_nodes(bias, tok, lens)
    np.testing.assert_array_equal(nodes, cases.model_nodes(name, rows))
    idx = cases.all_candidates(len(rows))
    assert cases.EOS in idx[0] and -1 in idx[0] and cases.V + 1 in idx[0]
    got = cases.host_terms(bias, nodes, idx)
    cases.same_bits(got, cases.model_terms(name, rows, idx))
    # through the class: what Transformer.beam_decode's host loop calls
    np.testing.assert_array_equal(bias.ast_nodes_host(tok, lens), nodes)
    cases.same_bits(bias.ast_terms_host(nodes, idx, cases.EOS), got)
    # a length beyond the stride is the stride, a negative one the empty row
    lens2 = lens.copy()
    lens2[1], lens2[2] = -4, LD + 9
    want2 = cases.model_nodes(name, [rows[0], [], tok[2].tolist()] + rows[3:])
    np.testing.assert_array_equal(cases.host_nodes(bias, tok, lens2), want2)
    # the other library's host twin is the same code
    np.testing.assert_array_equal(cases.host_nodes(bias, tok, lens, flavour="f16"), nodes)
    cases.same_bits(cases.host_terms(bias, nodes, idx, flavour="f16"), got)
    if name == "none":
        assert not nodes.any() and not got.view(np.int32).any()  # the root alone: every term is +0.0f


def test_the_cases_hold_what_they_are_meant_to():
    # a node of depth 31 and the completion of the 32-piece phrase
    bias = cases.bias_of("long")
    tok, lens = cases.pack([list(cases.LONG[:31]), list(cases.LONG)], 32)
    nodes = cases.host_nodes(bias, tok, lens)
    assert bias.depth[nodes[0]] == 31 and nodes[1] == 0
    t = cases.host_terms(bias, nodes[:1], np.array([[cases.LONG[31], cases.EOS, cases.IX["▁zz"]]], np.int32))
    assert t.tolist() == [[0.5, -15.5, -15.5]]
    # probe runs that wrap past slot 0, and a negative score
    wrap = cases.bias_of("probe_wrap")
    assert wrap.hash_bits == 1 and wrap.edges > 4 and (wrap.edge_keys[-4:] >= 0).any()
    assert (cases.bias_of("negative").value < 0).any()
    # the chain of three links: a candidate that only the fourth probed node knows
    chain = cases.bias_of("chain")
    tok, lens = cases.pack([cases.CHAIN_ROW], 8)
    n = cases.host_nodes(chain, tok, lens)
    assert chain.depth[n[0]] == 4
    assert cases.host_terms(chain, n, np.array([[cases.CHAIN_NEXT]], np.int32))[0, 0] == -4.0
    # eos as another id: the term of that id becomes the give-up, the old eos a piece like any other
    sp = cases.bias_of("shared_prefix")
    a, b, c = cases.ids("▁a b c")
    tok, lens = cases.pack([[a, b]], 4)
    n = cases.host_nodes(sp, tok, lens)
    idx = np.array([[c, cases.EOS]], np.int32)
    cases.same_bits(cases.host_terms(sp, n, idx, eos=c), cases.model_terms("shared_prefix", [[a, b]], idx, eos=c))
    assert cases.host_terms(sp, n, idx, eos=c)[0, 0] == -4.0 and cases.host_terms(sp, n, idx)[0, 0] == 2.0
    # a node outside the table counts as the root
    cases.same_bits(cases.host_terms(sp, np.array([sp.nodes, -1], np.int32), np.array([[a, cases.EOS]] * 2, np.int32)),
                    cases.host_terms(sp, np.array([0, 0], np.int32), np.array([[a, cases.EOS]] * 2, np.int32)))


def test_refusals_reached_without_a_gpu_call():
    bias = cases.bias_of("shared_prefix")
    good = bias.desc()
    L = hip.lib()
    tok, lens = cases.pack([[4, 5]], 4)
    node = np.full(3, cases.SENT_I, np.int32)
    idx = np.zeros((1, 2), np.int32)
    term = np.full(4, cases.SENT_F, np.float32)
    root = np.zeros(1, np.int32)

    def edited(**kw):
        d = hip.CnBiasDesc.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def nodes_host(desc=good, tok_=_ptr(tok), ld=4, lens_=_ptr(lens), n=1, out=_ptr(node)):
        return L.cn_ast_bias_nodes_host(C.byref(desc) if desc is not None else None, tok_, ld, lens_, n, out), L.cn_last_error()

    def terms_host(desc=good, node_=_ptr(root), idx_=_ptr(idx), n=1, K=2, out=_ptr(term)):
        return L.cn_ast_bias_terms_host(C.byref(desc) if desc is not None else None, node_, cases.EOS, idx_, n, K, out), L.cn_last_error()

    bad_descs = ((edited(slots=good.slots - 1), b"power of two"), (edited(slots=0), b"power of two"), (edited(nodes=-1), b"negative"),
                 (edited(hash_bits=33), b"hash_bits"), (edited(hash_bits=-1), b"hash_bits"), (edited(fail=None), b"null table"),
                 (edited(edge_keys=None), b"null table"), (edited(edge_child=None), b"null table"), (edited(value=None), b"null table"),
                 (edited(bank=None), b"null table"), (edited(reset=None), b"null table"))
    for call, kws in ((nodes_host, (dict(desc=None), dict(tok_=None), dict(lens_=None), dict(out=None), dict(n=0), dict(ld=0))),
                      (terms_host, (dict(desc=None), dict(node_=None), dict(idx_=None), dict(out=None), dict(n=0), dict(K=0)))):
        for kw in kws:
            rc, err = call(**kw)
            assert rc != 0 and (b"null" in err or b"< 1" in err), (kw, rc, err)
        for d, msg in bad_descs:
            rc, err = call(desc=d)
            assert rc != 0 and msg in err, (msg, rc, err)
    assert (node == cases.SENT_I).all() and (term == cases.SENT_F).all()
    ok_node, ok_term = np.full(1, cases.SENT_I, np.int32), np.full(2, cases.SENT_F, np.float32)
    assert nodes_host(out=_ptr(ok_node))[0] == 0 and terms_host(out=_ptr(ok_term))[0] == 0  # (the same calls, nothing wrong with them)
    assert ok_node[0] != cases.SENT_I and (ok_term != cases.SENT_F).all()

    # the device entries refuse the same arguments before they touch the GPU (the pointers are the host's: never dereferenced)
    att = np.zeros((1, cases.V), np.float32)
    for d, msg in bad_descs:
        assert L.cn_op_ast_bias_nodes(C.byref(d), _ptr(tok), 4, _ptr(lens), 1, _ptr(node), None) != 0 and msg in L.cn_last_error()
        assert L.cn_op_ast_bias_terms(C.byref(d), _ptr(node), cases.EOS, _ptr(idx), 1, 2, _ptr(term), None) != 0 and msg in L.cn_last_error()
        assert L.cn_op_logsoftmax_bias_topk(_ptr(att), 1, cases.V, 1.0, C.byref(d), _ptr(node), cases.EOS, 2, _ptr(idx), _ptr(term), None) != 0
        assert msg in L.cn_last_error()
    assert L.cn_op_ast_bias_nodes(None, _ptr(tok), 4, _ptr(lens), 1, _ptr(node), None) != 0
    assert L.cn_op_ast_bias_nodes(C.byref(good), _ptr(tok), 4, _ptr(lens), 0, _ptr(node), None) != 0
    assert L.cn_op_ast_bias_terms(C.byref(good), None, cases.EOS, _ptr(idx), 1, 2, _ptr(term), None) != 0
    assert L.cn_op_ast_bias_terms(C.byref(good), _ptr(node), cases.EOS, _ptr(idx), 1, 0, _ptr(term), None) != 0
    for kw in (dict(k=0), dict(k=33), dict(k=cases.V + 1), dict(V=8193), dict(T=0.0), dict(M=0)):
        a = dict(M=1, V=cases.V, T=1.0, k=2)
        a.update(kw)
        assert L.cn_op_logsoftmax_bias_topk(_ptr(att), a["M"], a["V"], a["T"], C.byref(good), _ptr(node), cases.EOS, a["k"], _ptr(idx), _ptr(term),
                                            None) != 0, kw
        assert L.cn_last_error()
    assert L.cn_op_logsoftmax_bias_topk(_ptr(att), 1, cases.V, 1.0, None, _ptr(node), cases.EOS, 2, _ptr(idx), _ptr(term), None) != 0
    # the handle entries: no handle is no AST model
    assert L.cn_ast_attach_bias(None, C.byref(good)) != 0 and b"autoregressive" in L.cn_last_error()
    assert L.cn_ast_attach_bias(None, None) != 0 and b"autoregressive" in L.cn_last_error()
    assert L.cn_ast_step_bias(None, 1, 0, None, None, None, None, 4, 1.0, 2, 0, cases.EOS, None, None, None, None, None) != 0
    assert b"cn_ast_begin" in L.cn_last_error()
    assert (node == cases.SENT_I).all() and (term == cases.SENT_F).all() and not idx.any()


# ---- the layers above ----------------------------------------------------------------------------------------------------------------
def test_the_parser_knows_the_flag_and_its_default():
    from cassnat_asr_public_amd.utils.parser import DecodeParser

    base = ["--task", "art", "--test_config", "c.yaml", "--data_path", "f.scp", "--resume_model", "m.mdl", "--result_file", "r.txt"]
    assert DecodeParser().get_args(base).hip_bias_search == "ctc"
    assert DecodeParser().get_args(base + ["--hip_bias", "names.txt"]).hip_bias_search == "ctc"
    assert DecodeParser().get_args(base + ["--hip_bias", "names.txt", "--hip_bias_search", "att"]).hip_bias_search == "att"
    with pytest.raises(SystemExit):
        DecodeParser().get_args(base + ["--hip_bias_search", "nat"])


@pytest.mark.parametrize("task,decode_type,extra,names", [("art", "ctc_only", dict(), "ctc_only"), ("art", "ctc_correct", dict(), "ctc_correct"),
                                                          ("cassnat", "ctc_only", dict(), "CassNATTask"), ("cassnat", "ctc_att", dict(), "CassNATTask"),
                                                          ("cassnat", "att_only", dict(), "CassNATTask"),
                                                          ("cassnat", "att_only", dict(sample_num=4), "CassNATTask")])
def test_tasks_refuse_att_on_paths_without_the_attention_beam_search(task, decode_type, extra, names):
    from cassnat_asr_public_amd.tasks import ArtTask, CassNATTask

    cls = CassNATTask if task == "cassnat" else ArtTask
    self = cls.__new__(cls)  # (decode looks at the arguments before it touches the loader or the model)
    self.test_loader = []
    for how in (dict(hip_bias="list.txt", hip_bias_model=None), dict(hip_bias="", hip_bias_model=cases.bias_of("interior"))):
        args = SimpleNamespace(decode_type=decode_type, hip_bias_search="att", beam_width=1, **how, **extra)
        with pytest.raises(NotImplementedError, match="hip_bias_search att") as e:
            cls.decode(self, args)
        assert names in str(e.value)


def test_without_the_flag_the_attention_beam_search_still_refuses_the_list():
    from cassnat_asr_public_amd.tasks import ArtTask

    self = ArtTask.__new__(ArtTask)
    self.test_loader = []
    for search in (dict(), dict(hip_bias_search="ctc")):
        args = SimpleNamespace(decode_type="ctc_att", hip_bias="list.txt", hip_bias_model=None, beam_width=1, **search)
        with pytest.raises(NotImplementedError, match="CTC prefix beam search") as e:
            ArtTask.decode(self, args)
        assert "ctc_att" in str(e.value)


def test_a_list_with_a_fused_language_model_is_refused_before_any_device_call():
    from cassnat_asr_public_amd.models.transformer import Transformer

    bias = cases.bias_of("interior")
    lm = SimpleNamespace(step_engine=lambda n: None)
    for kw, args in ((dict(bias=bias), SimpleNamespace(lm_weight=0.3)),
                     (dict(), SimpleNamespace(lm_weight=0.3, hip_bias_model=bias, hip_bias_search="att"))):
        with pytest.raises(NotImplementedError, match="hip_bias"):
            Transformer.beam_decode(None, None, None, None, args, lm, **kw)  # (model, features and vocabulary are None: nothing was touched)
    # with the default search the list is the CTC search's: beam_decode does not see it (and asks for its language model first)
    with pytest.raises(ValueError, match="lm_model"):
        Transformer.beam_decode(None, None, None, None, SimpleNamespace(lm_weight=0.3, hip_bias_model=bias), None)


def test_the_ctc_search_leaves_the_list_alone_when_it_is_the_attention_search_s():
    from cassnat_asr_public_amd.utils.beam_decode import ctc_beam_decode

    bias = cases.bias_of("interior")
    lm = SimpleNamespace(step_engine=lambda n: None)
    with pytest.raises(NotImplementedError, match="hip_bias"):
        ctc_beam_decode(None, None, None, None, None, SimpleNamespace(ctc_lm_weight=0.3, hip_bias_model=bias), lm)
    with pytest.raises(TypeError, match="ctc_lp"):  # (the next check: the list did not count)
        ctc_beam_decode(None, None, None, None, None, SimpleNamespace(ctc_lm_weight=0.3, hip_bias_model=bias, hip_bias_search="att", ctc_lp=None), lm)


def test_model_and_tables_name_nodes_alike():
    bias = cases.bias_of("interior")
    for i in range(bias.nodes):
        assert model.node_id(bias, model.node_of_id(bias, i)) == i and len(model.node_of_id(bias, i)) == bias.depth[i]
