"""The projecting form of the fused attention kernel (csrc/attention.hip, PROJ): the workgroup of an (entry, head) multiplies
LNn(x) by the Q|K|V tail units of the row-chain stream itself, so the chain launch in front of it ends with the LayerNorm and
the 3d-wide Q|K|V matrix never reaches memory.  The contract is bit-exactness:

* kernel level - a chain launch WITH the tail (blocked Q|K|V out) + the existing attention kernel, against a chain launch WITHOUT
  it (blocked LNn(x) out, x_mode bit 64) + cn_op_attention_proj, on the same x, ctx, weights and masks: the context rows and the
  residual stream must be EQUAL as raw words, in the bf16 and in the fp16 library;
* engine level - a decode with cn_decode_opts.reserved[2] (``args.hip_chain_qkv``: the two-launch form) against the default
  in one process: hypotheses, lengths, float64 scores, best_paths and enc_h must be equal.

Rows that nobody owns hold NaN when the attention kernels run: the rows of the last 32-row block past the launch's B * L rows
(written by the chain launch from a clamped row, overwritten here) and the buffers' padding behind them.  The rows between an
entry's ``kcap`` and L are a merged pass's padding rows: both kernels read them (their probability is exactly 0, and 0 * NaN is
NaN), so they keep the finite values the chain launch computed - as in a merged engine pass."""
import ctypes as C

import numpy as np
import pytest
import torch

from cassnat_asr_public_amd import hip, synth
from cassnat_asr_public_amd.models.cassnat import make_model

pytestmark = pytest.mark.gpu

D, H, B = 256, 4, 3
DFF = 256
PAD_ROWS = 128  # spare rows behind every blocked buffer
LIBS = {"bf16": (None, 1, torch.bfloat16), "fp16": ("f16", 4, torch.float16)}
LENGTHS = [1, 32, 33, 64, 65, 127, 250, 256]
MASKS = ["none", "suffix", "all_masked", "kcap"]


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def words(t):
    return t.cpu().contiguous().view(torch.int16).numpy()


def rows32(M):
    return -(-M // 32) * 32


def weights(seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    w = dict(wo=rn(D, D) / 16, bo=0.1 * rn(D), a1=1 + 0.1 * rn(D), b1n=0.1 * rn(D), w1=rn(DFF, D) / 16, b1=0.1 * rn(DFF),
             w2=rn(D, DFF) / 16, b2=0.1 * rn(D), na=1 + 0.1 * rn(D), nb=0.1 * rn(D), wt=rn(3 * D, D) / 8, bt=0.1 * rn(3 * D))
    return {k: v.contiguous() for k, v in w.items()}


def chain(L_, w, x, ctx, out, ldo, M, tail_n, x_mode):
    hip.check(L_.cn_op_chain(p(x), p(ctx), D, p(w["wo"]), p(w["bo"]), p(w["a1"]), p(w["b1n"]), p(w["w1"]), p(w["b1"]), p(w["w2"]),
                             p(w["b2"]), p(w["na"]), p(w["nb"]), p(w["wt"]), p(w["bt"]), p(out), ldo, M, DFF, tail_n, 1e-6, x_mode,
                             hip.current_stream()), "cn_op_chain", L_)


def nan_rows_blocked(buf, M, N):
    """NaN into rows M .. ceil(M / 32) * 32 - 1 of a blocked 16-bit buffer of N columns (either blocked layout: a 32-row block is
    N * 32 contiguous values and a row's values sit 8 at a time at (lane % 32 == row % 32) * 8 of every 512-value k-step / half)."""
    lo, hi = M, rows32(M)
    if lo == hi:
        return
    blk = buf[(lo >> 5) * 32 * N: hi * N].view(-1, 2, 32, 8)  # [piece][half][row % 32][8]
    blk[:, :, lo & 31:, :] = float("nan")


def masks_of(kind, L):
    """(keymask uint8 [B][L] or None, kcap int32 [B] or None)"""
    if kind == "none":
        return None, None
    if kind == "kcap":
        return None, torch.tensor([L, max(1, L - 7), max(1, L // 2)], dtype=torch.int32)
    km = torch.ones(B, L, dtype=torch.uint8)
    if kind == "suffix":
        km[1, L - max(1, L // 3):] = 0
    else:
        km[2, :] = 0
    return km, None


@pytest.fixture(scope="module")
def shared():
    return {"w": weights(1234)}


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("lib", sorted(LIBS))
def test_kernels_bit_exact(shared, lib, L):
    flavour, prec, dt = LIBS[lib]
    L_ = hip.lib(flavour)
    w = shared["w"]
    M = B * L
    g = torch.Generator().manual_seed(100 + L)
    x0 = (torch.randn(M, D, generator=g) * 2 + 0.3)
    ctx = torch.randn(M, D, generator=g).to(dt).cuda()
    nan16 = lambda n: torch.full((n,), float("nan"), dtype=dt, device="cuda")
    # ---- two-launch form: chain with the tail -> blocked Q|K|V
    xa = x0.clone().cuda()
    qkv = nan16((rows32(M) + PAD_ROWS) * 3 * D)
    chain(L_, w, xa, ctx, qkv, 3 * D, M, 3 * D, 16)
    # ---- projecting form: chain without it -> blocked LNn(x)
    xb = x0.clone().cuda()
    y = nan16((rows32(M) + PAD_ROWS) * D)
    chain(L_, w, xb, ctx, y, D, M, 0, 64)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(xa.cpu().numpy().view(np.int32), xb.cpu().numpy().view(np.int32))
    assert torch.isfinite(xa).all()
    assert torch.isfinite(qkv[: M // 32 * 32 * 3 * D].float()).all() and torch.isfinite(y[: M // 32 * 32 * D].float()).all()
    assert torch.isnan(qkv[rows32(M) * 3 * D:].float()).all() and torch.isnan(y[rows32(M) * D:].float()).all()
    nan_rows_blocked(qkv, M, 3 * D)
    nan_rows_blocked(y, M, D)
    for kind in MASKS:
        km, kcap = masks_of(kind, L)
        kmd = km.cuda() if km is not None else None
        kcd = kcap.cuda() if kcap is not None else None
        f = dict(B=B, H=H, Lq=L, Lk=L, scale=0.125, kcap_stride=1, ldo=D, o_blocked=1)
        if km is not None:
            f.update(keymask=kmd.data_ptr())
        if kcap is not None:
            f.update(kcap=kcd.data_ptr())
        oa = torch.full((rows32(M) * D,), 7.0, dtype=dt, device="cuda")
        ob = torch.full((rows32(M) * D,), 7.0, dtype=dt, device="cuda")
        da = hip.CnAttnDesc(**dict(f, Q=qkv.data_ptr(), K=qkv.data_ptr(), V=qkv.data_ptr(), O=oa.data_ptr(), q_blocked=1, kv_blocked=1,
                                   q_col=0, k_col=D, v_col=2 * D, q_n=3 * D, kv_n=3 * D, ldq=3 * D, ldk=3 * D, ldv=3 * D))
        hip.check(L_.cn_op_attention_desc(prec, C.byref(da), hip.current_stream()), "cn_op_attention_desc", L_)
        db = hip.CnAttnDesc(**dict(f, O=ob.data_ptr()))
        hip.check(L_.cn_op_attention_proj(prec, C.byref(db), p(y), p(w["wt"]), p(w["bt"]), hip.current_stream()), "cn_op_attention_proj", L_)
        torch.cuda.synchronize()
        a, b = words(oa), words(ob)
        np.testing.assert_array_equal(a, b, err_msg=f"{lib} L={L} {kind}")
        # owned rows: written and finite; the rows of the last block past M keep the sentinel
        o = ob.cpu().float().view(rows32(M) // 32, 16, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(rows32(M), D)
        assert torch.isfinite(o[:M]).all(), (lib, L, kind)
        assert (o[M:] == 7.0).all(), (lib, L, kind)
        assert not (o[:M] == 7.0).all(dim=1).any(), (lib, L, kind)


# ---------------------------------------------------------------------------------------------------------- engine level
FRAMES = [800, 790, 640, 523]  # T' = 200: the resident 8-wave self attention
MERGED = ([2, 2], [800, 620])  # a merged pass: the second batch has T' = 155 of the pass's 200


@pytest.fixture(scope="module")
def engine():
    args = synth.make_args("config2", N_enc=3, N_self_dec=1, N_mix_dec=1)
    args.hip_max_batch, args.hip_max_frames = 4, 1028
    state = synth.make_state(args, seed=0, blank_bias=0.35)
    return dict(args=args, state=state, models={})


def model_of(engine, prec):
    args = engine["args"]
    args.hip_precision, args.hip_capture = prec, False
    if prec not in engine["models"]:
        model = make_model(args.input_size, args).cuda()
        with torch.no_grad():
            for k, q in model.named_parameters():
                q.copy_(torch.from_numpy(engine["state"][k]))
        engine["models"][prec] = model
    return engine["models"][prec]


def both_forms(engine, prec, feats, sizes, **kw):
    model, args = model_of(engine, prec), engine["args"]
    got = []
    for chain_qkv in (True, False):
        args.hip_chain_qkv = chain_qkv
        out = model.decode_device(torch.from_numpy(feats), torch.from_numpy(sizes), args, 1, **kw)
        torch.cuda.synchronize()
        eng = model._engine
        got.append([t.cpu().numpy() for t in out[:3]] + [eng.fetch("best_paths"), eng.fetch("enc_h_live")])
    args.hip_chain_qkv = False
    return got


def assert_same(got, what):
    for name, a, b in zip(("hyp", "hyp_len", "score", "best_paths", "enc_h"), *got):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        assert np.isfinite(np.asarray(a, np.float64)).all(), (what, name)
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {name}")


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_engine_plain_pass(engine, prec):
    feats, sizes = synth.make_feats(len(FRAMES), FRAMES[0], 80, lengths=FRAMES, seed=501)
    got = both_forms(engine, prec, feats, sizes)
    assert got[0][3].shape[1] == 200
    assert_same(got, prec)


def test_engine_merged_pass(engine):
    rows, frames = MERGED
    fa, sa = synth.make_feats(2, frames[0], 80, lengths=[800, 700], seed=502)
    fb, sb = synth.make_feats(2, frames[1], 80, lengths=[620, 301], seed=503)
    feats = np.zeros((4, frames[0], 80), np.float32)
    feats[:2] = fa
    feats[2:, : frames[1]] = fb
    got = both_forms(engine, "bf16", feats, np.concatenate([sa, sb]), sub_rows=rows, sub_frames=frames)
    assert_same(got, "merged")
    # and the second batch is what a pass of its own gives (T' = 155: the projecting form there too)
    alone = both_forms(engine, "bf16", fb, sb)
    assert_same(alone, "second batch alone")
    n = min(alone[1][0].shape[1], got[1][0].shape[1])
    assert (alone[1][1] == got[1][1][2:]).all() and (alone[1][0][:, :n] == got[1][0][2:, :n]).all() and (alone[1][2] == got[1][2][2:]).all()


def test_engine_257_frames_keeps_the_two_launch_form(engine):
    """T' = 257: the self attention is the staged kernel, nothing is projected in it - the switch changes nothing."""
    feats, sizes = synth.make_feats(2, 1025, 80, lengths=[1025, 900], seed=504)
    got = both_forms(engine, "bf16", feats, sizes)
    assert got[0][3].shape[1] == 257
    assert_same(got, "T' = 257")
