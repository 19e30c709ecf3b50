"""Kernel-level tests of the packed decoder rows: the row plan against numpy, and the attention and row-chain
kernels on packed rows against the same kernels on padded rows - BITWISE on the rows an utterance owns, with the rows nobody
owns poisoned with NaN in the packed inputs."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from cassnat_asr_public_amd import hip
from test_gpu_attention import blk16_off, blocked_index, oblk_off
from test_gpu_kernels import _from_blocked, _from_blocked16, _hp, _to_blocked

pytestmark = pytest.mark.gpu
NAN = float("nan")
BF16 = hip.PRECISION["bf16"]


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ip(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------------------ row plan
def plan_numpy(ylen, U, hyp_stride, sub, meta, ymax):
    B = len(ylen)
    r = np.zeros(B, np.int64)
    for b in range(B):
        ulim = min(U, ymax) if ymax is not None else U
        if meta is not None or 0 < sub < B:
            b0, b1 = (meta[b][2], meta[b][3]) if meta is not None else ((b // sub) * sub, min((b // sub) * sub + sub, B))
            ulim = min(ulim, max([0] + [int(v) for v in ylen[b0:b1]]))
        r[b] = max(0, min(int(ylen[b]) + 1, ulim, hyp_stride - 1))
    return np.concatenate([[0], np.cumsum(r)])


def run_plan(ylen, U, hyp_stride, sub=0, meta=None, ymax=None):
    B = len(ylen)
    yd = torch.tensor(ylen, dtype=torch.int32).cuda()
    md = None if meta is None else torch.tensor(meta, dtype=torch.int32).cuda()
    xd = None if ymax is None else torch.tensor([ymax], dtype=torch.int32).cuda()
    out = torch.full((B + 1,), -7, dtype=torch.int32).cuda()
    hip.check(hip.lib().cn_op_row_plan(p(yd), B, U, hyp_stride, sub, p(md), p(xd), p(out), hip.current_stream()), "cn_op_row_plan")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_row_plan_against_numpy():
    rng = np.random.default_rng(5)
    # whole pass; a pass of one utterance; a predicted U above and below the true maximum
    for ylen, U, ymax in [([7, 3, 1, 7, 5], 7, None), ([4], 4, None), ([1], 1, None), ([9, 2, 6], 40, 9), ([9, 2, 6], 5, 9)]:
        np.testing.assert_array_equal(run_plan(ylen, U, U + 1, ymax=ymax), plan_numpy(ylen, U, U + 1, 0, None, ymax))
    # equal-sized batches: one whose utterances are all empty (the EOS row alone), one of a single utterance at the end
    ylen = [12, 5, 9, 1, 1, 1, 30, 2, 3, 17]
    np.testing.assert_array_equal(run_plan(ylen, 30, 31, sub=3), plan_numpy(ylen, 30, 31, 3, None, None))
    assert run_plan(ylen, 30, 31, sub=3)[3:7].tolist() == [12 + 6 + 10, 29, 30, 31]  # (the empty batch: one row each)
    # the batches of a merged pass (any sizes), with a batch without any row at all (use_trigger off: ylen 0) and a batch of one
    meta = [[0, 0, 0, 2]] * 2 + [[0, 0, 2, 5]] * 3 + [[0, 0, 5, 6]] + [[0, 0, 6, 10]] * 4
    ylen = [5, 8, 0, 0, 0, 11, 3, 3, 1, 2]
    got = run_plan(ylen, 11, 12, meta=meta, ymax=11)
    np.testing.assert_array_equal(got, plan_numpy(ylen, 11, 12, 0, meta, 11))
    assert got[2] == got[5] and got[6] - got[5] == 11
    # more utterances than one scan chunk holds, batches of 7, a hypothesis buffer that binds
    ylen = rng.integers(1, 90, size=700).tolist()
    np.testing.assert_array_equal(run_plan(ylen, 89, 60, sub=7), plan_numpy(ylen, 89, 60, 7, None, None))


# ------------------------------------------------------------------------------------------------------------ attention
def pack16(x16, N, rows):
    """Row-major 16-bit (M, N) -> the blocked buffer of `rows` rows (the others NaN)."""
    buf = torch.full((-(-rows // 32) * 32 * N,), NAN, dtype=x16.dtype)
    buf[blocked_index(x16.shape[0], N, blk16_off).reshape(-1)] = x16.reshape(-1)
    return buf


def launch(f, keep, row_off=None, kv_packed=0):
    desc = hip.CnAttnDesc(**f)
    L = hip.lib()
    if row_off is None:
        hip.check(L.cn_op_attention_desc(BF16, C.byref(desc), hip.current_stream()), "cn_op_attention_desc")
    else:
        hip.check(L.cn_op_attention_packed(BF16, C.byref(desc), p(row_off), kv_packed, hip.current_stream()), "cn_op_attention_packed")
    torch.cuda.synchronize()
    del keep


def gather_rows(x, U, r):
    """padded (B * U, n) -> packed (sum r, n) rows, then NaN up to the capacity B * U."""
    B = len(r)
    own = torch.cat([x[b * U: b * U + r[b]] for b in range(B)])
    return torch.cat([own, torch.full((B * U - own.shape[0], x.shape[1]), NAN, dtype=x.dtype)])


def out_rows(O, blocked, M, d):
    o = O.cpu()
    return o[blocked_index(M, d, oblk_off)] if blocked else o.view(-1, d)[:M]


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("U,r,klen", [
    (40, [1, 40, 33, 2, 17], [1, 39, 33, 1, 16]),                # 2-wave form
    (100, [65, 64, 1, 100, 31, 97], [64, 63, 1, 100, 30, 96]),   # 4-wave form; key tiles 1 and 2
    (150, [150, 3, 129, 64, 128], [149, 2, 128, 64, 127]),       # 8-wave form; three key tiles, waves and workgroups that leave
    (300, [300, 70, 257, 5], [299, 69, 256, 4]),                 # more than 256 keys: the staged form
])
def test_packed_self_attention_equals_padded_bitwise(U, r, klen, blocked):
    B, H = len(r), 4
    d = 64 * H
    g = torch.Generator().manual_seed(U + B)
    X = torch.randn(B * U, 3 * d, generator=g).to(torch.bfloat16)
    kl = torch.tensor(klen, dtype=torch.int32).cuda()
    roff = torch.tensor(np.concatenate([[0], np.cumsum(r)]), dtype=torch.int32).cuda()
    outs = []
    for packed in (False, True):
        x = gather_rows(X, U, r) if packed else X
        rows = B * U
        if blocked:
            Xd = pack16(x, 3 * d, rows).cuda()
            O = torch.full((-(-rows // 32) * 32 * d,), NAN, dtype=torch.bfloat16).cuda()
            f = dict(Q=ip(Xd), K=ip(Xd), V=ip(Xd), q_blocked=1, kv_blocked=1, q_col=0, k_col=d, v_col=2 * d, q_n=3 * d, kv_n=3 * d,
                     o_blocked=1)
        else:
            Xd = x.cuda()
            O = torch.full((rows, d), NAN, dtype=torch.bfloat16).cuda()
            f = dict(Q=ip(Xd), K=ip(Xd) + 2 * d, V=ip(Xd) + 4 * d)
        f.update(O=ip(O), ldq=3 * d, ldk=3 * d, ldv=3 * d, ldo=d, B=B, H=H, Lq=U, Lk=U, klen=ip(kl), kcap_stride=1, scale=0.125)
        launch(f, [Xd, kl], roff if packed else None, 1)
        outs.append(out_rows(O, blocked, rows, d))
    padded, packed = outs
    lo = 0
    for b in range(B):
        own = packed[lo: lo + r[b]]
        assert torch.isfinite(own.float()).all(), b
        assert torch.equal(own.view(torch.int16), padded[b * U: b * U + r[b]].view(torch.int16)), b
        lo += r[b]
    assert torch.isnan(packed[lo:].float()).all()  # nothing is written behind the rows that exist


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("U,Lk,r", [(40, 77, [1, 40, 12, 33]), (100, 250, [65, 1, 100, 31, 97]), (150, 300, [150, 3, 129, 64])])
def test_packed_source_attention_equals_padded_bitwise(U, Lk, r, blocked):
    """Only the query rows, their intervals and the outputs move; utterance 1's trigger intervals are all empty (every key
    masked: the uniform row of the reference), and a key mask cuts the frames of the shorter utterances."""
    B, H = len(r), 4
    d = 64 * H
    g = torch.Generator().manual_seed(U + Lk)
    Q = torch.randn(B * U, d, generator=g).to(torch.bfloat16)
    KV = torch.randn(B * Lk, 2 * d, generator=g).to(torch.bfloat16)
    frames = [Lk - 7 * b for b in range(B)]
    km = torch.zeros(B, Lk, dtype=torch.uint8)
    iv = torch.zeros(B, Lk + 1, 4, dtype=torch.int32)
    for b in range(B):
        km[b, : frames[b]] = 1
        for u in range(U):
            s = (u * frames[b]) // U
            iv[b, u] = torch.tensor([s, min(frames[b], s + 3), frames[b] - 1 if u == r[b] - 1 else 0, frames[b] if u == r[b] - 1 else 0])
    iv[1] = 0
    kmd, ivd = km.cuda(), iv.cuda()
    roff = torch.tensor(np.concatenate([[0], np.cumsum(r)]), dtype=torch.int32).cuda()
    outs = []
    for packed in (False, True):
        q = gather_rows(Q, U, r) if packed else Q
        rows = B * U
        if blocked:
            Qd, KVd = pack16(q, d, rows).cuda(), pack16(KV, 2 * d, B * Lk).cuda()
            O = torch.full((-(-rows // 32) * 32 * d,), NAN, dtype=torch.bfloat16).cuda()
            f = dict(Q=ip(Qd), K=ip(KVd), V=ip(KVd), q_blocked=1, kv_blocked=1, q_col=0, k_col=0, v_col=d, q_n=d, kv_n=2 * d, o_blocked=1)
        else:
            Qd, KVd = q.cuda(), KV.cuda()
            O = torch.full((rows, d), NAN, dtype=torch.bfloat16).cuda()
            f = dict(Q=ip(Qd), K=ip(KVd), V=ip(KVd) + 2 * d)
        f.update(O=ip(O), ldq=d, ldk=2 * d, ldv=2 * d, ldo=d, B=B, H=H, Lq=U, Lk=Lk, keymask=ip(kmd), intervals=ip(ivd), iv_stride=Lk + 1,
                 kcap_stride=1, scale=0.125)
        launch(f, [Qd, KVd, kmd, ivd], roff if packed else None, 0)
        outs.append(out_rows(O, blocked, rows, d))
    padded, packed = outs
    lo = 0
    for b in range(B):
        own = packed[lo: lo + r[b]]
        assert torch.isfinite(own.float()).all(), b
        assert torch.equal(own.view(torch.int16), padded[b * U: b * U + r[b]].view(torch.int16)), b
        lo += r[b]
    assert torch.isnan(packed[lo:].float()).all()


def test_packed_attention_refuses_what_it_does_not_define():
    d = 256
    X = torch.zeros(64, 3 * d, dtype=torch.bfloat16).cuda()
    O = torch.zeros(64, d, dtype=torch.bfloat16).cuda()
    roff = torch.tensor([0, 3, 9], dtype=torch.int32).cuda()
    km = torch.ones(2, 32, dtype=torch.uint8).cuda()
    f = dict(Q=ip(X), K=ip(X) + 2 * d, V=ip(X) + 4 * d, O=ip(O), ldq=3 * d, ldk=3 * d, ldv=3 * d, ldo=d, B=2, H=4, Lq=32, Lk=32,
             kcap_stride=1, scale=0.125)
    L = hip.lib()
    for extra in (dict(keymask=ip(km)), dict(kv_mod=1), dict(Lk=16)):
        desc = hip.CnAttnDesc(**dict(f, **extra))
        assert L.cn_op_attention_packed(BF16, C.byref(desc), p(roff), 1, hip.current_stream()) != 0
        assert "packed" in L.cn_last_error().decode()
    desc = hip.CnAttnDesc(**f)
    assert L.cn_op_attention_packed(BF16, C.byref(desc), None, 1, hip.current_stream()) != 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ row chain
@pytest.mark.parametrize("x_mode", [0, 3 | 16])  # row-major stream and tail; blocked stream in and out with a blocked tail
@pytest.mark.parametrize("total", [1, 127, 129])
def test_chain_with_the_row_count_on_the_device_equals_the_host_count_bitwise(total, x_mode):
    """The launch is sized for 300 rows (three workgroups); `total` of them exist.  Rows behind them are NaN in the inputs (in
    the blocked forms: behind the last 32-row block that holds a row - the block's spare rows are finite, as the query fill
    leaves them)."""
    cap, d, dff, tail_n = 300, 256, 512, 768
    g = torch.Generator().manual_seed(total)
    rn = lambda *s: torch.randn(*s, generator=g)
    x, ctx = rn(cap, d) * 2 + 0.3, rn(cap, d).to(torch.bfloat16)
    wo, bo = (rn(d, d) / 16).contiguous(), 0.1 * rn(d)
    a1, b1n = 1 + 0.1 * rn(d), 0.1 * rn(d)
    w1, b1 = (rn(dff, d) / 16).contiguous(), 0.1 * rn(dff)
    w2, b2 = (rn(d, dff) / math.sqrt(dff)).contiguous(), 0.1 * rn(d)
    na, nb = 1 + 0.1 * rn(d), 0.1 * rn(d)
    wt, bt = (rn(tail_n, d) / 16).contiguous(), 0.1 * rn(tail_n)
    blk = bool(x_mode & 1)
    keep_rows = -(-total // 32) * 32 if blk else total
    xs, cs = x.clone(), ctx.clone()
    xs[keep_rows:], cs[total:] = NAN, NAN
    rows_dev = torch.tensor([total], dtype=torch.int32).cuda()
    res = []
    for on_device in (False, True):
        M = cap if on_device else total
        xin = xs[:M] if on_device else xs[:total]
        xd = (_to_blocked(xin) if blk else xin.clone()).cuda()
        ctxd = cs[:M].contiguous().cuda()
        rows_out = -(-M // 32) * 32 if x_mode & 16 else M
        out = torch.full((rows_out, tail_n), NAN, dtype=torch.bfloat16).cuda()
        args = [p(xd), p(ctxd), d, _hp(wo), _hp(bo), _hp(a1), _hp(b1n), _hp(w1), _hp(b1), _hp(w2), _hp(b2), _hp(na), _hp(nb), _hp(wt),
                _hp(bt), p(out), tail_n, M, dff, tail_n, 1e-6, x_mode]
        if on_device:
            hip.check(hip.lib().cn_op_chain_rows(*args, p(rows_dev), hip.current_stream()), "cn_op_chain_rows")
        else:
            hip.check(hip.lib().cn_op_chain(*args, hip.current_stream()), "cn_op_chain")
        torch.cuda.synchronize()
        nrb = -(-M // 32)
        xo = xd.cpu()
        xo = _from_blocked(xo.reshape(-1)[: nrb * 32 * d].view(nrb, 32, 64, 4), M) if blk else xo.view(-1, d)[:M]
        oo = _from_blocked16(out.cpu(), M, tail_n) if x_mode & 16 else out.cpu()[:M]
        res.append((xo, oo))
    (x_host, o_host), (x_dev, o_dev) = res
    assert torch.isfinite(x_dev[:total]).all() and torch.isfinite(o_dev[:total].float()).all()
    assert torch.equal(x_dev[:total].view(torch.int32), x_host[:total].view(torch.int32))
    assert torch.equal(o_dev[:total].view(torch.int16), o_host[:total].view(torch.int16))
    # the workgroups behind the rows that exist wrote nothing
    first_idle = -(-total // 128) * 128
    assert torch.isnan(x_dev[first_idle:]).all() and torch.isnan(o_dev[first_idle:].float()).all()
