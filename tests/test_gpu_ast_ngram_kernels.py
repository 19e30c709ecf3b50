"""The kernels of the AST beam search's word n-gram fusion (csrc/ast_ngram.hip, csrc/rowops.hip), one at a time, against the numpy
model of tests/ast_ngram_model.py and against float32 compositions of kernels that have their own tests: cn_op_ast_ngram_adds (bit
for bit the host entry and the model), cn_op_ast_ngram_terms, cn_op_logsoftmax_class_topk (bit for bit log-softmax + fl32(w * term),
stable descending order) and the refusals of cn_ast_attach_ngram."""
import ctypes as C

import numpy as np
import pytest
import torch

import ast_ngram_cases as cases
import ast_ngram_model as model_of
from cassnat_asr_public_amd import hip, synth
from cassnat_asr_public_amd.models import make_transformer
from test_gpu_ast_kernels import gather_rows, p, stream

pytestmark = pytest.mark.gpu

N, LD = 70, 41


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ================================================================================================================= adds
@pytest.mark.parametrize("order", cases.ORDERS)
def test_adds_are_the_host_entry_and_the_model_bit_for_bit(order):
    lm, model = cases.lm_of(order)
    lm.cuda()
    rows = cases.crafted(LD)
    rows += cases.random_rows(np.random.RandomState(order), N - len(rows), LD)
    assert len(rows) == N
    tok, lens = cases.pack(rows, LD)
    out = torch.full((2 * N + 8,), cases.SENT, dtype=torch.float32, device="cuda")
    tok_d, lens_d = dev(tok), dev(lens)
    hip.check(hip.lib().cn_op_ast_ngram_adds(C.byref(lm.desc(lm.device)), p(tok_d), LD, p(lens_d), N, cases.EOS, p(out), stream()))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[2 * N:] == cases.SENT).all()  # nothing behind the rows' pairs is written
    got = out[:2 * N].reshape(N, 2)
    cases.same_bits(got, cases.host_adds(lm, tok, lens))
    cases.same_bits(got, cases.model_adds(model, rows))


def test_adds_of_rows_longer_than_a_wave_and_of_clamped_lengths():
    """130 ids are three chunks of the wave's scan: words span the chunk borders; a length beyond the stride is the stride."""
    lm, model = cases.lm_of(3)
    lm.cuda()
    ld = 130
    rows = cases.random_rows(np.random.RandomState(8), 12, ld)
    rows[0] = (rows[0] + [cases.IX["▁a"]] * ld)[:ld]
    rows[1] = [cases.IX["▁ab"]] + [cases.IX["c"]] * (ld - 1)  # one word of 130 pieces
    rows[2] = [cases.IX["c"]] * 63 + [cases.IX["▁a"]] + [cases.IX["b"]] * 64 + [cases.IX["▁"], cases.IX["▁b"]]
    tok, lens = cases.pack(rows, ld)
    lens[3], lens[4] = ld + 50, -2
    rows[3], rows[4] = tok[3].tolist(), []
    out = torch.full((24 + 8,), cases.SENT, dtype=torch.float32, device="cuda")
    tok_d, lens_d = dev(tok), dev(lens)
    hip.check(hip.lib().cn_op_ast_ngram_adds(C.byref(lm.desc(lm.device)), p(tok_d), ld, p(lens_d), 12, cases.EOS, p(out), stream()))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[24:] == cases.SENT).all()
    cases.same_bits(out[:24].reshape(12, 2), cases.model_adds(model, rows))
    cases.same_bits(out[:24].reshape(12, 2), cases.host_adds(lm, tok, lens))


def test_adds_on_the_colliding_key_model():
    from ctc_ngram_cases import collision_case

    case = collision_case()
    lm, model = cases.lm_of(1, case.hash_bits)
    lm.cuda()
    spell = [[cases.IX["▁zz"]] + [cases.IX[c] for c in w[2:]] if w.startswith("zz") else [cases.IX["▁" + w[0]]] + [cases.IX[c] for c in w[1:]]
             for w in case.hit[:4]]
    rows = spell + [s + [cases.IX["▁"]] for s in spell] + cases.crafted(LD)
    tok, lens = cases.pack(rows, LD)
    out = torch.empty(len(rows), 2, dtype=torch.float32, device="cuda")
    tok_d, lens_d = dev(tok), dev(lens)
    hip.check(hip.lib().cn_op_ast_ngram_adds(C.byref(lm.desc(lm.device)), p(tok_d), LD, p(lens_d), len(rows), cases.EOS, p(out), stream()))
    torch.cuda.synchronize()
    cases.same_bits(out.cpu().numpy(), cases.model_adds(model, rows))


# ================================================================================================================ terms
@pytest.mark.parametrize("K", [1, 15, 32])
def test_terms_at_the_candidates(K):
    lm, model = cases.lm_of(3)
    lm.cuda()
    rows = cases.crafted(LD)
    n = len(rows)
    adds = cases.model_adds(model, rows)
    assert (adds[:, 0] != 0).any() and (adds[:, 0] == 0).any()
    rng = np.random.RandomState(K)
    idx = rng.randint(0, cases.V, (n, K)).astype(np.int32)
    special = [cases.EOS, cases.IX["▁a"], cases.IX["bc"], cases.BLANK, cases.SOS, cases.IX["▁"], cases.IX["▁zz"], -1]
    for r in range(n):  # every row meets eos, word-starting and continuation pieces, blank and sos
        for j in range(K):
            if (r + j) % 3 == 0 or K == 1:
                idx[r, j] = special[(r + j // 3) % len(special)]
    starts = model_of.starts_of(cases.VOCAB)
    assert np.array_equal(starts, lm._host["piece_starts"].numpy())
    out = torch.full((n * K + 8,), cases.SENT, dtype=torch.float32, device="cuda")
    adds_d, idx_d = dev(adds), dev(idx)
    hip.check(hip.lib().cn_op_ast_ngram_terms(p(lm._dev[lm.device]["piece_starts"]), p(adds_d), cases.EOS, p(idx_d), n, K, p(out), stream()))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[n * K:] == cases.SENT).all()
    want = model_of.terms(adds, starts, cases.EOS, idx)
    cases.same_bits(out[:n * K].reshape(n, K), want)
    for c in (cases.EOS, cases.IX["▁a"], cases.IX["bc"], cases.BLANK, cases.SOS):
        assert (idx == c).any()
    assert (want[idx == cases.BLANK] == 0).all() and (want[idx == cases.SOS] == 0).all() and (want[idx == cases.IX["bc"]] == 0).all()


# ==================================================================================================== class top-k (rowops)
def class_rows(M, V, seed, eos):
    """att logits, starts, adds.  Row 0: the attention top-k are word-starting pieces and a_word pushes them out; row 1: exact ties
    (equal logits, equal class: the lower index wins) ; row 2: quantised logits; row 3: eos wins only through a_eos; row 4: zero adds."""
    g = np.random.default_rng(seed)
    att = (g.standard_normal((M, V)) * 3).astype(np.float32)
    starts = (g.random(V) < 0.4).astype(np.uint8)
    starts[eos] = 0
    adds = -(g.integers(0, 513, (M, 2)) / 64.0).astype(np.float32)
    adds[5:, :] *= np.float32(1.37)  # (not dyadic: every operation is still a defined float32 one)
    att[0, eos] = -30.0
    top = np.argsort(-att[0], kind="stable")[:32]
    starts[top] = 1
    starts[eos] = 0
    adds[0] = (-40.0, -1.5)
    tie = [j for j in (7, 3, V - 1) if j != eos]
    starts[tie] = 0
    att[1, tie] = att[1].max() + 1.0
    att[2] = np.round(att[2] * 2) / 2
    assert eos != 5
    att[3, 5] = att[3].max() + 1.0  # the best begins a word; eos is second, half a unit behind
    att[3, eos] = att[3, 5] - 0.5
    starts[5] = 1
    adds[3] = (-3.0, 0.0)
    adds[4] = 0.0
    return att, starts, adds


@pytest.mark.parametrize("V", [28, 1028, 5000, 8192])
def test_logsoftmax_class_topk_bit_for_bit(V):
    """val must be fl32(log_softmax(att / T)[c] + fl32(w * term(c))) with the log-probabilities as cn_op_logsoftmax_gather computes
    them (the same partition and order of maximum and log-sum-exp), idx its stable descending order (ties: lower index)."""
    M, eos = 12, cases.EOS
    att, starts, adds = class_rows(M, V, seed=V, eos=eos)
    att_d, starts_d, adds_d = dev(att), dev(starts), dev(adds)
    every = np.tile(np.arange(V, dtype=np.int32), (M, 1))
    term = model_of.terms(adds, starts, eos, every)
    L = hip.lib()
    for T in (1.0, 1.3):
        a_lp = gather_rows((att / np.float32(T)).astype(np.float32) if T != 1.0 else att, every)
        for w in (1e-3, 0.5, 2.0):
            fused = (a_lp + np.float32(w) * term).astype(np.float32)  # float32, two roundings (numpy does not contract)
            order = np.argsort(-fused, axis=1, kind="stable")
            for k in (1, 20, 32):
                if k > V:
                    continue
                idx = torch.empty(M, k, dtype=torch.int32, device="cuda")
                val = torch.empty(M, k, dtype=torch.float32, device="cuda")
                hip.check(L.cn_op_logsoftmax_class_topk(p(att_d), M, V, T, p(starts_d), p(adds_d), eos, w, k, p(idx), p(val), stream()))
                torch.cuda.synchronize()
                idx, val = idx.cpu().numpy(), val.cpu().numpy()
                assert np.array_equal(idx, order[:, :k]), (V, k, T, w, np.argwhere(idx != order[:, :k])[:4].tolist())
                want = np.take_along_axis(fused, order[:, :k], 1)
                assert np.array_equal(val.view(np.int32), want.view(np.int32)), (V, k, T, w)
                plain = np.argsort(-a_lp, axis=1, kind="stable")
                if w >= 0.5 and V > 64:  # the attention top-k is pushed out by the class term
                    assert not set(idx[0].tolist()) & set(plain[0, :k].tolist())
                tie = [j for j in (3, 7, V - 1) if j != eos]
                assert idx[1, :len(tie)].tolist() == tie[:k]  # exact ties: lower index first
                if w >= 0.5:  # eos is second by attention and first only through a_eos
                    assert plain[3, 0] != eos and idx[3, 0] == eos
                # zero adds: the plain kernel's output, bit for bit (here on the zero row, below on all rows)
                assert idx[4].tolist() == plain[4, :k].tolist()
    zero = dev(np.zeros((M, 2), np.float32))
    for T in (1.0, 1.3):
        for k in (1, min(32, V)):
            a, b = (torch.empty(M, k, dtype=torch.int32, device="cuda") for _ in range(2))
            va, vb = (torch.empty(M, k, dtype=torch.float32, device="cuda") for _ in range(2))
            hip.check(L.cn_op_logsoftmax_class_topk(p(att_d), M, V, T, p(starts_d), p(zero), eos, 0.5, k, p(a), p(va), stream()))
            hip.check(L.cn_op_logsoftmax_topk(p(att_d), M, V, T, k, p(b), p(vb), stream()))
            torch.cuda.synchronize()
            assert torch.equal(a, b) and torch.equal(va.view(torch.int32), vb.view(torch.int32)), (V, T, k)


def test_class_topk_refusals():
    L = hip.lib()
    x = torch.zeros(2, 40, device="cuda")
    st = torch.zeros(40, dtype=torch.uint8, device="cuda")
    ad = torch.zeros(2, 2, device="cuda")
    idx = torch.zeros(2, 40, dtype=torch.int32, device="cuda")
    val = torch.zeros(2, 40, device="cuda")
    for V, k in ((40, 0), (40, 33), (20, 21), (8193, 4)):
        assert L.cn_op_logsoftmax_class_topk(p(x), 2, V, 1.0, p(st), p(ad), 2, 0.5, k, p(idx), p(val), stream()) != 0
        assert b"k <= min(32, V)" in L.cn_last_error()
    assert L.cn_op_logsoftmax_class_topk(p(x), 2, 40, 1.0, None, p(ad), 2, 0.5, 4, p(idx), p(val), stream()) != 0
    assert L.cn_op_logsoftmax_class_topk(p(x), 2, 40, 1.0, p(st), None, 2, 0.5, 4, p(idx), p(val), stream()) != 0


# ================================================================================================================ attach
def test_attach_refusals():
    lm, _ = cases.lm_of(3)
    lm.cuda()
    args = synth.make_args_ast("tiny_ast", vocab_size=cases.V)
    args.hip_precision = "fp32"
    ast = make_transformer(args.input_size, args).cuda()
    eng = ast.engine(2, 64)
    L = eng.L
    good = lm.desc(lm.device)

    def changed(**kw):
        d = hip.CnNgramDesc.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def refused(handle, desc, scale, what):
        assert L.cn_ast_attach_ngram(handle, C.byref(desc), scale) != 0
        assert what in L.cn_last_error().decode(), L.cn_last_error()

    refused(eng.handle, changed(order=0), 0.5, "order 0 is outside 1 .. 8")
    refused(eng.handle, changed(order=9), 0.5, "order 9 is outside 1 .. 8")
    refused(eng.handle, changed(vocab=cases.V + 1), 0.5, "vocabulary")
    refused(eng.handle, changed(gram_slots=good.gram_slots - 2), 0.5, "powers of two")
    refused(eng.handle, changed(word_slots=3), 0.5, "powers of two")
    refused(eng.handle, good, float("nan"), "lm_scale must be a number")
    # a handle that is no AST model: the TransformerLM's
    from cassnat_asr_public_amd.models.lm import make_model as make_lm

    lm_args = synth.make_args_lm("tiny_lm", vocab_size=cases.V)
    lm_args.hip_precision = "fp32"
    tlm = make_lm(lm_args).cuda()
    refused(tlm.step_engine(2).handle, good, 0.5, "autoregressive model")
    assert L.cn_ast_attach_ngram(None, C.byref(good), 0.5) != 0
    # and the attach, then the detach, are accepted
    eng.ast_attach_ngram(good, 0.5)
    eng.ast_attach_ngram(None)
