"""The two kernels of the CASS-NAT finish loop with word n-gram fusion (csrc/nat_ngram.hip) one at a time: cn_op_nat_class_topk against
numpy, bit for bit, and cn_op_nat_ngram_finish on its tables against the serial host entry from full rows (which
tests/test_nat_ngram_host.py pins to the numpy model): every beam, its order and its float64 score exact.  B = 3: one utterance at
ylen 0, one whose last row lies at its zlen (read as zero), one that consumes every row."""
import ctypes as C

import numpy as np
import pytest
import torch

import ast_ngram_model as model_of
import nat_ngram_cases as cases
import nat_ngram_model as nn
from cassnat_asr_public_amd import hip
from test_gpu_ast_kernels import p, stream

pytestmark = pytest.mark.gpu

B = 3
US, VS, BEAMS, ORDERS = (1, 2, 5, 40), (40, 5000, 8192), (1, 3, 16), (1, 2, 3, 5)
_ROWS = {}


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared rows are read-only)


def rows(U, V, grid=False):
    """One set of rows per shape, shared by the tests and never written."""
    key = (U, V, grid)
    if key not in _ROWS:
        a = cases.rows_of(B, U, V, seed=7, grid=grid)
        a.setflags(write=False)
        _ROWS[key] = a
    return _ROWS[key]


def class_topk(att_d, last_d, zlen_d, U, V, starts_d, k, pad=8):
    n = B * U * 2 * k
    idx = torch.full((n + pad,), cases.SENT_I, dtype=torch.int32, device="cuda")
    val = torch.full((n + pad,), cases.SENT_F, dtype=torch.float32, device="cuda")
    ev = torch.full((B * U + pad,), cases.SENT_F, dtype=torch.float32, device="cuda")
    hip.check(hip.lib().cn_op_nat_class_topk(p(att_d), p(last_d), p(zlen_d), B, U, V, p(starts_d), cases.EOS, k, p(idx), p(val), p(ev), stream()),
              "cn_op_nat_class_topk")
    return idx, val, ev


@pytest.mark.parametrize("k", BEAMS)
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("U", US)
def test_class_topk_is_numpy_bit_for_bit(U, V, k):
    grid = (U + k) % 2 == 0  # rows on a grid of quarters: ties inside a class, decided by the index
    att = rows(U, V, grid)
    starts = model_of.starts_of(cases.vocab_of(V))
    ylen = cases.lens_of(B, U)
    last = np.minimum(ylen, U - 1).astype(np.int32)
    last[2] = U + 5  # beyond the rows: clamped to U - 1
    idx, val, ev = class_topk(dev(att), dev(last), dev(ylen), U, V, dev(starts), k)
    torch.cuda.synchronize()
    idx, val, ev = idx.cpu().numpy(), val.cpu().numpy(), ev.cpu().numpy()
    n = B * U * 2 * k
    assert (idx[n:] == cases.SENT_I).all() and (val[n:] == cases.SENT_F).all() and (ev[B * U:] == cases.SENT_F).all()
    idx, val, ev = idx[:n].reshape(B, U, 2, k), val[:n].reshape(B, U, 2, k), ev[:B * U].reshape(B, U)
    zero_rows = 0
    for b in range(B):
        for i in range(U):
            if i > min(last[b], U - 1):  # not consumed: not written
                assert (idx[b, i] == cases.SENT_I).all() and (val[b, i] == cases.SENT_F).all() and ev[b, i] == cases.SENT_F
                continue
            zero = i >= ylen[b]
            zero_rows += zero
            wi, wv, we = nn.class_tables(np.zeros(V, np.float32) if zero else att[b, i], starts, cases.EOS, k)
            assert idx[b, i].tolist() == wi.tolist(), (b, i)
            assert val[b, i].view(np.int32).tolist() == wv.view(np.int32).tolist() and ev[b, i].view(np.int32) == we.view(np.int32), (b, i)
            if zero:  # the lowest indices of each class, value 0
                assert all(wi[c, j] < wi[c, j + 1] or wi[c, j + 1] < 0 for c in (0, 1) for j in range(k - 1)) and (wv[wi >= 0] == 0).all()
    assert zero_rows >= 1
    if V == 40 and k == 16:
        assert (idx[2, U - 1, 0] == -1).any() and np.isneginf(val[2, U - 1, 0][idx[2, U - 1, 0] == -1]).all()  # a class smaller than k pads


def finish_on_device(lm, att, ylen, ymax, bw, scale, lp, use_lp, zero, L=None):
    """cn_op_nat_class_topk then cn_op_nat_ngram_finish; beams as cases.run_host gives them."""
    _, U, V = att.shape
    L = ymax + 1 if L is None else L
    lm.cuda()
    last_d = dev(np.minimum(ylen, ymax - 1).astype(np.int32))
    idx, val, ev = class_topk(dev(att), last_d, dev(ylen) if zero else None, U, V, lm._dev[lm.device]["piece_starts"], bw)
    pad = 8
    hist = torch.zeros(B * U * bw * 2, dtype=torch.int32, device="cuda")
    hyp = torch.full((B * bw * L + pad,), cases.SENT_I, dtype=torch.int32, device="cuda")
    hlen = torch.full((B * bw + pad,), cases.SENT_I, dtype=torch.int32, device="cuda")
    sc = torch.full((B * bw + pad,), cases.SENT_F, dtype=torch.float64, device="cuda")
    hip.check(hip.lib().cn_op_nat_ngram_finish(C.byref(lm.desc(lm.device)), float(np.float32(scale)), p(idx), p(val), p(ev), p(last_d), B, U, bw, cases.EOS,
                                               cases.SOS, cases.PAD, use_lp, float(lp), p(hist), p(hyp), L, p(hlen), p(sc), stream()),
              "cn_op_nat_ngram_finish")
    torch.cuda.synchronize()
    hyp, hlen, sc = hyp.cpu().numpy(), hlen.cpu().numpy(), sc.cpu().numpy()
    assert (hyp[B * bw * L:] == cases.SENT_I).all() and (hlen[B * bw:] == cases.SENT_I).all() and (sc[B * bw:] == cases.SENT_F).all()
    return cases.beams_of(hyp[:B * bw * L].reshape(B, bw, L), hlen[:B * bw].reshape(B, bw), sc[:B * bw].reshape(B, bw))


@pytest.mark.parametrize("bw", BEAMS)
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("order", ORDERS)
def test_finish_is_the_host_entry(order, V, bw):
    """Every U of the setup; the length penalty on and off and rows past zlen read as zero or not, in turn."""
    lm, _ = cases.lm_for(order, V)
    for n, U in enumerate(US):
        att = rows(U, V, grid=(n + order) % 2 == 1)
        ylen = cases.lens_of(B, U)
        use_lp, zero = (n + bw) % 2, (n + order + bw) % 2 == 0
        got = finish_on_device(lm, att, ylen, U, bw, 0.5, 0.25, use_lp, zero)
        want = cases.run_host(lm, att, ylen, U, bw, 0.5, lp=0.25, use_lp=use_lp, zlen=ylen if zero else None)
        cases.same_beams(got, want)
        assert [len(u[0]["hyp"]) for u in got] == [min(int(y), U - 1) + 2 for y in ylen]


def test_finish_with_a_shorter_ymax_and_a_longer_row():
    lm, _ = cases.lm_for(3, 40)
    att, ylen = rows(40, 40), np.array([40, 3, 17], np.int32)
    got = finish_on_device(lm, att, ylen, 11, 5, 0.5, 0.1, 1, True, L=20)
    cases.same_beams(got, cases.run_host(lm, att, ylen, 11, 5, 0.5, lp=0.1, zlen=ylen, L=20))
    assert [len(u[0]["hyp"]) for u in got] == [12, 5, 12]


@pytest.mark.parametrize("bw", [3, 16])
def test_finish_on_the_colliding_key_model_and_on_a_model_that_rounds(bw):
    (lm, _), case = cases.collision_lm(40)
    att, ylen = cases.spelled_rows(case.hit[:4], 40)
    U = att.shape[1]
    got = finish_on_device(lm, att, ylen, U, bw, 0.5, 0.1, 1, False)
    cases.same_beams(got, cases.run_host(lm, att, ylen, U, bw, 0.5, lp=0.1))
    plain = cases.lm_for(1, 40)[0]
    assert got != cases.run_host(plain, att, ylen, U, bw, 0.5, lp=0.1)   # the collisions were met
    lm, _ = cases.plain_lm(5000)
    att, ylen = rows(40, 5000), cases.lens_of(B, 40)
    scale = float(np.float32(0.3 * np.log(10.0)))
    for use_lp in (0, 1):
        got = finish_on_device(lm, att, ylen, 40, bw, scale, 0.1, use_lp, True)
        cases.same_beams(got, cases.run_host(lm, att, ylen, 40, bw, scale, lp=0.1, use_lp=use_lp, zlen=ylen))


def test_refusals_launch_nothing():
    L = hip.lib()
    lm, _ = cases.lm_for(3, 40)
    lm.cuda()
    U, V, k = 2, 40, 3
    att_d, last_d = dev(rows(U, V)), dev(np.array([1, 1, 1], np.int32))
    starts_d = lm._dev[lm.device]["piece_starts"]
    n = B * U * 2 * k
    idx = torch.full((n,), cases.SENT_I, dtype=torch.int32, device="cuda")
    val = torch.full((n,), cases.SENT_F, dtype=torch.float32, device="cuda")
    ev = torch.full((B * U,), cases.SENT_F, dtype=torch.float32, device="cuda")

    def topk(Bv=B, Uv=U, Vv=V, kv=k, eos=cases.EOS, att=att_d):
        return L.cn_op_nat_class_topk(p(att), p(last_d), None, Bv, Uv, Vv, p(starts_d), eos, kv, p(idx), p(val), p(ev), stream())

    for kw, what in ((dict(Vv=8193), b"8192"), (dict(kv=0), b"beam_width"), (dict(kv=17), b"beam_width"), (dict(Vv=2), b"beam_width"),
                     (dict(eos=-1), b"eos"), (dict(eos=V), b"eos"), (dict(Bv=0), b"positive"), (dict(Uv=0), b"positive"), (dict(att=None), b"null")):
        assert topk(**kw) != 0 and what in L.cn_last_error(), (kw, L.cn_last_error())
    hist = torch.zeros(B * U * k * 2, dtype=torch.int32, device="cuda")
    hyp = torch.full((B * k * 3,), cases.SENT_I, dtype=torch.int32, device="cuda")
    hlen = torch.full((B * k,), cases.SENT_I, dtype=torch.int32, device="cuda")
    sc = torch.full((B * k,), cases.SENT_F, dtype=torch.float64, device="cuda")

    def changed(**kw):
        d = hip.CnNgramDesc.from_buffer_copy(lm.desc(lm.device))
        for key, v in kw.items():
            setattr(d, key, v)
        return d

    def finish(desc=None, bw=k, eos=cases.EOS, scale=0.5, lp=0.0, Lm=3, Bv=B, Uv=U, hist_t=hist):
        d = desc if desc is not None else lm.desc(lm.device)
        return L.cn_op_nat_ngram_finish(C.byref(d), scale, p(idx), p(val), p(ev), p(last_d), Bv, Uv, bw, eos, cases.SOS, cases.PAD, 1, lp, p(hist_t),
                                        p(hyp), Lm, p(hlen), p(sc), stream())

    for kw, what in ((dict(desc=changed(vocab=8193)), b"8192"), (dict(desc=changed(order=9)), b"order 9"), (dict(desc=changed(gram_slots=48)), b"powers of two"),
                     (dict(desc=changed(gram_keys=None)), b"null table"), (dict(bw=0), b"beam_width"), (dict(bw=17), b"beam_width"),
                     (dict(eos=40), b"eos"), (dict(scale=float("nan")), b"numbers"), (dict(lp=float("nan")), b"numbers"), (dict(Lm=0), b"max_len"),
                     (dict(Bv=0), b"positive"), (dict(Uv=0), b"positive"), (dict(hist_t=None), b"null")):
        assert finish(**kw) != 0 and what in L.cn_last_error(), (kw, L.cn_last_error())
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == cases.SENT_I).all() and (hyp.cpu().numpy() == cases.SENT_I).all() and (sc.cpu().numpy() == cases.SENT_F).all()
    assert topk() == 0 and finish() == 0
    torch.cuda.synchronize()
    assert (hlen.cpu().numpy() == 3).all()  # last = 1, max_len 3: every hypothesis has its three tokens
