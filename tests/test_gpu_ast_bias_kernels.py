"""The kernels of the AST beam search's phrase biasing (csrc/ast_bias.hip), one at a time through the C ABI of both libraries:
cn_op_ast_bias_nodes and cn_op_ast_bias_terms against the host twins and the numpy model of tests/ast_bias_model.py, bit for bit;
cn_op_logsoftmax_bias_topk against numpy - the log-probabilities of cn_op_logsoftmax_gather (the same partition and order of maximum
and log-sum-exp), fl32(x + term) with the model's terms, stable descending order - idx and val bit for bit; the empty list against
cn_op_logsoftmax_topk; the refusals, which leave the outputs alone."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ast_bias_cases as cases
import ast_bias_model as model
from cassnat_asr_public_amd import hip, synth
from cassnat_asr_public_amd.models import make_transformer
from cassnat_asr_public_amd.models.bias import BiasList
from test_gpu_ast_kernels import gather_rows, p, stream

pytestmark = pytest.mark.gpu

LD = 75
LENGTHS = (0, 1, 40, 75)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def rows_for(name, n):
    """n rows of lengths 0 / 1 / 40 / 75 in turn over the set's pieces, planted phrases among them; the case list's rows come first."""
    phrases = cases.SETS[name][0]
    rng = np.random.RandomState(n + len(name))
    used = sorted({c for ph in phrases for c in ph} | {cases.IX["▁zz"], cases.IX["a"]})
    plants = [list(q) for q in cases.ctc_cases.plants(phrases)]
    rows = [r for r in cases.rows_of(name, 41)][:max(0, n - 8)]
    while len(rows) < n:
        want, row = LENGTHS[len(rows) % 4], []
        while len(row) < want:
            row += plants[rng.randint(len(plants))] if rng.rand() < 0.5 else [int(rng.choice(used))]
        rows.append(row[:want])
    return rows[:n]


# ======================================================================================================== nodes and terms
@pytest.mark.parametrize("flavour", [None, "f16"])
@pytest.mark.parametrize("n,K", [(1, 1), (3, 5), (65, 32), (640, 5)])
def test_nodes_and_terms_are_the_host_twins_and_the_model_bit_for_bit(n, K, flavour):
    L = hip.lib(flavour)
    for name in ("shared_prefix", "interior", "long", "negative", "probe_wrap", "chain", "none"):
        bias = cases.bias_of(name).cuda()
        desc = bias.desc(bias.device)
        rows = rows_for(name, n) if n > 1 else [list(cases.CHAIN_ROW if name == "chain" else cases.LONG[:31])]
        tok, lens = cases.pack(rows, LD)
        if n >= 65:  # a length beyond the stride is the stride, a negative one the empty row
            lens[1], lens[2] = -4, LD + 9
            rows = [rows[0], [], tok[2].tolist()] + rows[3:]
        assert {len(r) for r in rows} >= (set(LENGTHS) if n >= 65 else set())
        out = torch.full((n + 8,), cases.SENT_I, dtype=torch.int32, device="cuda")
        tok_d, lens_d = dev(tok), dev(lens)
        hip.check(L.cn_op_ast_bias_nodes(C.byref(desc), p(tok_d), LD, p(lens_d), n, p(out), stream()), "cn_op_ast_bias_nodes", L)
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert (out[n:] == cases.SENT_I).all()  # nothing behind the rows' nodes is written
        nodes = cases.host_nodes(bias, tok, lens, flavour=flavour)
        np.testing.assert_array_equal(out[:n], nodes)
        if n <= 65:
            np.testing.assert_array_equal(nodes, cases.model_nodes(name, rows))
        if name == "long" and n >= 65:
            assert (np.array(bias.depth)[nodes] >= 8).any()
        # terms at K candidates: ids of the vocabulary, eos, ids outside it
        idx = cases.candidates(n, K, np.random.RandomState(n + K))
        if K >= 5:
            assert (idx == cases.EOS).any() and (idx < 0).any()
        tout = torch.full((n * K + 8,), cases.SENT_F, dtype=torch.float32, device="cuda")
        nodes_d, idx_d = dev(nodes), dev(idx)
        hip.check(L.cn_op_ast_bias_terms(C.byref(desc), p(nodes_d), cases.EOS, p(idx_d), n, K, p(tout), stream()), "cn_op_ast_bias_terms", L)
        torch.cuda.synchronize()
        tout = tout.cpu().numpy()
        assert (tout[n * K:] == cases.SENT_F).all()
        got = tout[:n * K].reshape(n, K)
        cases.same_bits(got, cases.host_terms(bias, nodes, idx, flavour=flavour))
        if n <= 65:
            cases.same_bits(got, cases.model_terms(name, rows, idx))
        if name == "none":
            assert not got.view(np.int32).any()
        # the Python wrappers are the same calls
        if flavour is None and n == 3:
            assert torch.equal(hip.ast_bias_nodes(desc, tok_d, lens_d), nodes_d)
            cases.same_bits(hip.ast_bias_terms(desc, nodes_d, cases.EOS, idx_d).cpu().numpy(), got)


# ============================================================================================================ fused top-k
@functools.lru_cache(maxsize=None)
def topk_case(kind, V):
    """(BiasList, phrases, rows): the set `kind` of the case list ("long": a node of depth 31; "chain": a failure chain of three
    links) and, where the vocabulary is larger than the pieces', random phrases of 1 to 4 ids spread over it, dyadic scores; the rows are
    hypotheses at the root, inside matches, at depth 31 / on the chain, behind a completed phrase."""
    phrases = dict(cases.SETS[kind][0])
    rng = np.random.RandomState(V + len(kind))
    if V > cases.V:
        for _ in range(24):
            ids = tuple(int(t) for t in rng.randint(cases.V, V, rng.randint(1, 5)))
            phrases[ids] = float(rng.choice([0.5, 2.0, 3.0, -1.0]))
        first = next(q for q in phrases if q[0] >= cases.V and len(q) > 1)
        phrases[(first[0], V - 1)] = 2.0  # the last id of the vocabulary continues a match
    bias = BiasList.from_phrases(phrases)
    deep = list(cases.LONG[:31]) if kind == "long" else list(cases.CHAIN_ROW)
    rows = [[], deep, deep[:2], [cases.IX["▁zz"]], deep[:1]]
    for q in sorted(phrases)[:40]:
        rows += [list(q[:-1]), list(q), list(q[:1])]
    return bias, phrases, rows


def every_term(phrases, row, V, eos):
    """The model's terms of a hypothesis for every id of the vocabulary: ids no phrase holds all break the match alike, so one of them
    is asked and stands for the rest."""
    used = sorted({c for q in phrases for c in q if c < V})
    foreign = next(c for c in range(V - 1, -1, -1) if c not in used and c != eos)
    asked = used + [eos, foreign]
    got = model.terms(row, phrases, eos, V, asked)
    out = np.full(V, got[-1], np.float32)
    out[asked] = got
    return out


@pytest.mark.parametrize("V", [28, 40, 5000, 8192])
def test_logsoftmax_bias_topk_bit_for_bit(V):
    eos = cases.EOS
    for kind, M, k, T, flavour in (("long", 1, 1, 1.0, None), ("chain", 2, 3, 1.3, None), ("long", 5, 16, 1.0, "f16"), ("chain", 40, 32, 1.3, None),
                                   ("long", 40, 32, 1.0, None)):
        k = min(k, V)
        L = hip.lib(flavour)
        bias, phrases, rows = topk_case(kind, V)
        bias.cuda()
        desc = bias.desc(bias.device)
        # M == 1: the deep row; else the case's rows in turn, the root row first
        rows = [rows[1]] if M == 1 else [rows[i % len(rows)] for i in range(M)]
        tok, lens = cases.pack(rows, LD)
        nodes = cases.host_nodes(bias, tok, lens)
        depth = np.array(bias.depth)[nodes]
        if kind == "long":
            assert (depth == 31).any()
        else:
            n, links = int(nodes[0 if M == 1 else 1]), 0
            while n:
                n, links = int(bias.fail[n]), links + 1
            assert links >= 4  # three shorter matches before the root
        if M > 1:
            assert (depth == 0).any() and (depth > 0).any()
        g = np.random.default_rng(V + M)
        att = (g.standard_normal((M, V)) * 3).astype(np.float32)
        term = np.stack([every_term(phrases, r, V, eos) for r in rows])
        # the eos entry gives the open match up
        np.testing.assert_array_equal(term[:, eos], np.where(nodes != 0, -bias.value[nodes], np.float32(0.0)))
        # the piece that completes the deep match is outside the attention top-k and enters it through its term
        nxt = cases.LONG[31] if kind == "long" else cases.IX["cb"]
        deep_rows = [r for r in range(M) if depth[r] >= 4 and rows[r] == rows[0 if M == 1 else 1]]
        for r in deep_rows:
            assert term[r, nxt] - term[r].min() >= 10.0
            att[r, nxt] = np.sort(att[r])[::-1][min(k, V - 1)] - 2.0
        # exact ties: equal logits, far above the rest, on ids no phrase holds (equal terms): the lower index wins
        used = {c for q in phrases for c in q}
        tie = [c for c in range(V - 1, -1, -1) if c not in used and c != eos][:3][::-1]
        if M > 1:
            att[-1, tie] = att[-1].max() + 40.0
        if M >= 5:
            att[2] = np.round(att[2] * 2) / 2  # quantised logits: ties all over the row
        every = np.tile(np.arange(V, dtype=np.int32), (M, 1))
        a_lp = gather_rows((att / np.float32(T)).astype(np.float32) if T != 1.0 else att, every)
        fused = (a_lp + term).astype(np.float32)  # float32, one rounding
        order = np.argsort(-fused, axis=1, kind="stable")
        idx = torch.full((M * k + 8,), cases.SENT_I, dtype=torch.int32, device="cuda")
        val = torch.full((M * k + 8,), cases.SENT_F, dtype=torch.float32, device="cuda")
        att_d, nodes_d = dev(att), dev(nodes)
        hip.check(L.cn_op_logsoftmax_bias_topk(p(att_d), M, V, T, C.byref(desc), p(nodes_d), eos, k, p(idx), p(val), stream()),
                  "cn_op_logsoftmax_bias_topk", L)
        torch.cuda.synchronize()
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        assert (idx[M * k:] == cases.SENT_I).all() and (val[M * k:] == cases.SENT_F).all()
        idx, val = idx[:M * k].reshape(M, k), val[:M * k].reshape(M, k)
        assert np.array_equal(idx, order[:, :k]), (V, kind, M, k, np.argwhere(idx != order[:, :k])[:4].tolist())
        want = np.take_along_axis(fused, order[:, :k], 1)
        assert np.array_equal(val.view(np.int32), want.view(np.int32)), (V, kind, M, k)
        plain = np.argsort(-a_lp, axis=1, kind="stable")
        if M > 1:
            assert idx[-1, :min(k, 3)].tolist() == tie[:k]
        if k >= 3:  # the terms decide something
            for r in deep_rows:
                if r != M - 1:
                    assert nxt in idx[r] and (nxt not in plain[r, :k] or k == V) and idx[r].tolist() != plain[r, :k].tolist()
        if flavour is None and M == 2:
            i2, v2 = hip.logsoftmax_bias_topk(att_d, T, desc, nodes_d, eos, k)
            assert np.array_equal(i2.cpu().numpy(), idx) and np.array_equal(v2.cpu().numpy().view(np.int32), val.view(np.int32))


@pytest.mark.parametrize("V", [28, 5000])
def test_an_empty_list_is_logsoftmax_topk_in_every_bit(V):
    M = 7
    att = dev((np.random.default_rng(V).standard_normal((M, V)) * 3).astype(np.float32))
    none = cases.bias_of("none").cuda()
    bare = hip.CnBiasDesc(slots=1, nodes=1)  # the root alone without tables: nothing is read
    nodes = dev(np.array([0, 3, -1, 0, 100, 0, 1], np.int32))
    for flavour in (None, "f16"):
        L = hip.lib(flavour)
        for desc in (none.desc(none.device), bare):
            for T in (1.0, 1.3):
                for k in (1, min(32, V)):
                    a, b = (torch.empty(M, k, dtype=torch.int32, device="cuda") for _ in range(2))
                    va, vb = (torch.empty(M, k, dtype=torch.float32, device="cuda") for _ in range(2))
                    hip.check(L.cn_op_logsoftmax_bias_topk(p(att), M, V, T, C.byref(desc), p(nodes), cases.EOS, k, p(a), p(va), stream()), "", L)
                    hip.check(L.cn_op_logsoftmax_topk(p(att), M, V, T, k, p(b), p(vb), stream()), "", L)
                    torch.cuda.synchronize()
                    assert torch.equal(a, b) and torch.equal(va.view(torch.int32), vb.view(torch.int32)), (V, T, k)


def test_every_node_at_the_root_of_a_list_whose_pieces_the_row_lacks_is_logsoftmax_topk_too():
    """Rows at the root of a real list: only the listed first pieces get a term; with those entries far down the output is the plain
    kernel's."""
    V, M, k = 40, 3, 8
    bias = cases.bias_of("shared_prefix").cuda()
    att = (np.random.default_rng(5).standard_normal((M, V)) * 3).astype(np.float32)
    att[:, [q[0] for q in bias.phrases]] = -40.0
    att_d, nodes = dev(att), dev(np.zeros(M, np.int32))
    L = hip.lib()
    a, b = (torch.empty(M, k, dtype=torch.int32, device="cuda") for _ in range(2))
    va, vb = (torch.empty(M, k, dtype=torch.float32, device="cuda") for _ in range(2))
    hip.check(L.cn_op_logsoftmax_bias_topk(p(att_d), M, V, 1.0, C.byref(bias.desc(bias.device)), p(nodes), cases.EOS, k, p(a), p(va), stream()))
    hip.check(L.cn_op_logsoftmax_topk(p(att_d), M, V, 1.0, k, p(b), p(vb), stream()))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(va.view(torch.int32), vb.view(torch.int32))


# =============================================================================================================== refusals
def test_refusals_leave_the_outputs_alone():
    L = hip.lib()
    bias = cases.bias_of("shared_prefix").cuda()
    good = bias.desc(bias.device)
    x = torch.zeros(2, 40, device="cuda")
    node = torch.zeros(2, dtype=torch.int32, device="cuda")
    tok = torch.zeros(2, 4, dtype=torch.int32, device="cuda")
    idx = torch.full((2, 40), cases.SENT_I, dtype=torch.int32, device="cuda")
    val = torch.full((2, 40), cases.SENT_F, dtype=torch.float32, device="cuda")
    out = torch.full((2,), cases.SENT_I, dtype=torch.int32, device="cuda")
    bad = hip.CnBiasDesc.from_buffer_copy(good)
    bad.slots = good.slots - 1
    for V, k in ((40, 0), (40, 33), (20, 21), (8193, 4)):
        assert L.cn_op_logsoftmax_bias_topk(p(x), 2, V, 1.0, C.byref(good), p(node), 2, k, p(idx), p(val), stream()) != 0
        assert b"k <= min(32, V)" in L.cn_last_error()
    assert L.cn_op_logsoftmax_bias_topk(p(x), 2, 40, 1.0, C.byref(bad), p(node), 2, 4, p(idx), p(val), stream()) != 0
    assert L.cn_op_logsoftmax_bias_topk(p(x), 2, 40, 1.0, None, p(node), 2, 4, p(idx), p(val), stream()) != 0
    assert L.cn_op_logsoftmax_bias_topk(p(x), 2, 40, 1.0, C.byref(good), None, 2, 4, p(idx), p(val), stream()) != 0
    assert L.cn_op_logsoftmax_bias_topk(p(x), 2, 40, float("nan"), C.byref(good), p(node), 2, 4, p(idx), p(val), stream()) != 0
    assert L.cn_op_ast_bias_terms(C.byref(bad), p(node), 2, p(idx), 2, 4, p(val), stream()) != 0 and b"power of two" in L.cn_last_error()
    assert L.cn_op_ast_bias_terms(C.byref(good), p(node), 2, None, 2, 4, p(val), stream()) != 0
    assert L.cn_op_ast_bias_terms(C.byref(good), p(node), 2, p(idx), 0, 4, p(val), stream()) != 0
    assert L.cn_op_ast_bias_nodes(C.byref(bad), p(tok), 4, p(node), 2, p(out), stream()) != 0 and b"power of two" in L.cn_last_error()
    assert L.cn_op_ast_bias_nodes(C.byref(good), p(tok), 0, p(node), 2, p(out), stream()) != 0
    assert L.cn_op_ast_bias_nodes(C.byref(good), None, 4, p(node), 2, p(out), stream()) != 0
    torch.cuda.synchronize()
    assert (idx == cases.SENT_I).all() and (val == cases.SENT_F).all() and (out == cases.SENT_I).all()


def test_attach_and_step_refusals():
    bias = cases.bias_of("shared_prefix").cuda()
    good = bias.desc(bias.device)
    args = synth.make_args_ast("tiny_ast", vocab_size=cases.V)
    args.hip_precision = "fp32"
    ast = make_transformer(args.input_size, args).cuda()
    eng = ast.engine(2, 64)
    L = eng.L

    def changed(**kw):
        d = hip.CnBiasDesc.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def refused(handle, desc, what):
        assert L.cn_ast_attach_bias(handle, C.byref(desc)) != 0
        assert what in L.cn_last_error().decode(), L.cn_last_error()

    refused(eng.handle, changed(slots=good.slots - 2), "power of two")
    refused(eng.handle, changed(nodes=-1), "negative")
    refused(eng.handle, changed(hash_bits=40), "hash_bits")
    refused(eng.handle, changed(value=None), "null table")
    # a handle that is no AST model: the TransformerLM's
    from cassnat_asr_public_amd.models.lm import make_model as make_lm

    lm_args = synth.make_args_lm("tiny_lm", vocab_size=cases.V)
    lm_args.hip_precision = "fp32"
    tlm = make_lm(lm_args).cuda()
    refused(tlm.step_engine(2).handle, good, "autoregressive model")
    # the step entry before cn_ast_begin, and without a list
    z = torch.zeros(2, 8, dtype=torch.int32, device="cuda")
    with pytest.raises(hip.HipError, match="cn_ast_begin|attached"):
        eng.ast_step_bias(0, z[:, 0], z[:, 0], z, z.to(torch.uint8), 1.0, 2, 0, cases.EOS, z[:, 0], z[:, :2], z[:, :2].float())
    # and the attach, then the detach, are accepted
    eng.ast_attach_bias(good)
    eng.ast_attach_bias(None)
