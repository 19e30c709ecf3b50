"""A float64 model of one launch of the row-chain kernel (csrc/chain.hip) with a per-element error bound, the buffers of every
launch form the engine uses, and the checks a launch must pass.  Shared by the kernel test (test_gpu_chain.py), the CPU test that
shows the checks would catch what a kernel can get wrong (test_chain_model.py) and the argument test (test_chain_args.py).

The operation (include/cassnat_hip.h, cn_chain_desc):

    x += Wo . ctx + bo                      if ctx is given
    x += W2 . act(W1 . LN1(x) + b1) + b2    if d_ff > 0 (act: ReLU or Swish)
    y = LNn(x); out = Wt . y + bt (the tail) or y itself; ln_out = y as well where asked for

LayerNorm is the reference's (oracle.cassnat_oracle.layer_norm): unbiased std, eps added to the std.  The operands are what the
kernel sees: ctx as its 16-bit values, weights rounded to the library's operand type (bf16 / fp16); biases and LayerNorm vectors
stay fp32.  The roundings the kernel applies on the way - LayerNorm outputs and hidden activations rounded to the operand, fp32
accumulation, the output's 16-bit rounding - are NOT replayed by the model: the bound covers them.

Two checks per launch (check_launch):

* |out - fp64| <= bound for every live element of x, ln_out and the tail.  The bound is a worst case: operand unit roundoff times
  sum |w| |a| for each rounded intermediate, gamma(K) for each fp32 accumulation of K terms (with a factor 2 for what an MFMA's
  internal adder may do differently from K roundings), the first product's bound carried through the activation (Lipschitz
  constant 1 / 1.1) and the second product, x's bound carried through LNn, half an output ulp.
* the aggregate check.  Worst-case bounds are loose against coherent errors (a bias of a few tenths of a percent stays inside
  them), so the model also runs an EMULATION: the same operation with every intermediate rounding applied and float64
  accumulation.  The RMS of (result - fp64) over an output's live elements must stay within RATIO[layout] of the yardstick

      sqrt(rms(emulation - fp64)^2 + rms(fp32 accumulation)^2),

  whose second term is a random-walk estimate of what fp32 accumulation adds, EPS sqrt(K) (|x| + rms of the row's products + |bias|)
  per product (K roundings of partial sums of about that size, independent of each other): it only matters
  where no operand rounding feeds an output (x after the output projection alone), where the emulation's own error is one fp32
  rounding.  The yardstick is never a second launch.
"""
import numpy as np
import torch

from attention_model import EPS, LAYOUTS, gamma, out_ulp

D = 256
SENTINEL = 7.0
NAN = float("nan")
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
U_OP = {"bf16": 2.0 ** -9, "fp16": 2.0 ** -12}  # unit roundoff of the 16-bit operand (half an ulp, relative)
U_SUB = {"bf16": 0.0, "fp16": 2.0 ** -25}       # half a subnormal step of IEEE half (absolute)
SWISH_LIP = 1.1                                  # max |d/dv v sigmoid(v)| = 1.0998
LIBS = [n for n in ("bf16", "fp16") if n in LAYOUTS]

# what the aggregate check allows: RMS(result - fp64) / yardstick.  Measured on the MI355X over every case of CASES (the table in
# docs/KERNEL_NOTES.md, "Row-chain kernel: float64 tests of every launch form"): at most 1.005 (bf16) and 1.035 (fp16) over every
# output of every form - the kernel's error IS the operand roundings the emulation applies, fp32 accumulation adds next to nothing.
# Of the listed mistakes only the two 0.2 % LayerNorm ones stay inside the per-element bounds; in the fp16 layout they move the
# ratio to 5.8 at the least (test_chain_model.py prints and asserts it), in the bf16 layout to 1.11 .. 1.39 (at the size of the
# operand's own roundoff: reported, not required).  fp16: 1.25 leaves a factor 1.2 above the measurement and 4.6 below the
# smallest mistake; bf16: 1.1, twenty times the excess that was measured.
RATIO = {"bf16": 1.1, "fp16": 1.25}

MISTAKES = ("ln1_biased_std", "lnn_biased_std", "ln1_eps_in_var", "lnn_eps_in_var", "no_b1", "no_b2", "no_bo", "no_bt",
            "no_residual_attn", "no_residual_ffn", "act_swapped", "lnn_uses_ln1_vectors", "ldctx_ignored", "clamp_to_capacity",
            "store_at_capacity", "xin_blk_chunks", "xout_blk_chunks", "ctx_blk_chunks", "out_blk_chunks", "ln_blk_chunks",
            "tail_tile_shifted")


def rows32(M):
    return -(-M // 32) * 32


# ================================================================================================ layouts
def blk16_off(m, c, N):
    """cn_blk16_off (common.h): byte offset of the 16-byte chunk at (row m, column c % 8 == 0) of a blocked [M][N] matrix."""
    return ((((m >> 5) * (N >> 5) + (c >> 5)) << 1) + ((c >> 4) & 1)) * 1024 + ((((c >> 3) & 1) << 5) + (m & 31)) * 16


def oblk_off(m, c, ldo):
    """The o_blocked order (AttnArgs): byte offset of the chunk at (row m, channel c % 8 == 0)."""
    return ((m >> 5) * (ldo // 16) + (c >> 4)) * 1024 + (((c >> 3) & 1) * 32 + (m & 31)) * 16


def _grid(M, N):
    return np.arange(M)[:, None], np.arange(N)[None, :]


def rm_index(M, N, ld):
    """(M, N) element index of a row-major matrix with row stride ld."""
    m, c = _grid(M, N)
    return torch.from_numpy(m * ld + c)


def blk16_index(M, N, ldo=None):
    """Columns 0 .. N - 1 of the blocked 16-bit matrix of ldo columns the tail is written as (out_blocked)."""
    m, c = _grid(M, N)
    return torch.from_numpy(blk16_off(m, c - c % 8, N if ldo is None else ldo) // 2 + c % 8)


def oblk_index(M):
    """The blocked ctx (ctx_blocked: the attention kernel's o_blocked output of 256 columns)."""
    m, c = _grid(M, D)
    return torch.from_numpy(oblk_off(m, c - c % 8, D) // 2 + c % 8)


def lnblk_index(M):
    """The blocked LNn(x) (ln_blocked): per 32-row block [16 k-steps][lane = row % 32 + 32 h][8], value j of (ks, h) being channel
    32 (ks / 2) + 16 (ks % 2) + 8 (j / 4) + 4 h + j % 4."""
    m, c = _grid(M, D)
    ks, h, j = 2 * (c >> 5) + ((c >> 4) & 1), (c >> 2) & 1, 4 * ((c >> 3) & 1) + (c & 3)
    return torch.from_numpy((m >> 5) * 8192 + ks * 512 + ((m & 31) + 32 * h) * 8 + j)


def xblk_index(M):
    """The blocked fp32 residual stream: 32-row blocks of [32 pieces i][64 lanes][4 floats], lane = row % 32 + 32 h holding channels
    32 (i / 4) + 8 (i % 4) + 4 h + (0..3)."""
    m, c = _grid(M, D)
    i, h, e = 4 * (c >> 5) + ((c >> 3) & 3), (c >> 2) & 1, c & 3
    return torch.from_numpy((m >> 5) * 8192 + i * 256 + ((m & 31) + 32 * h) * 4 + e)


def to_blocked_x(x):
    """[M][256] -> blocked x, rows padded to 32 with zeros (as test_gpu_kernels.py states it, by permutation)."""
    nrb = rows32(x.shape[0]) // 32
    xp = torch.zeros(nrb * 32, D, dtype=x.dtype)
    xp[:x.shape[0]] = x
    return xp.view(nrb, 32, 8, 4, 2, 4).permute(0, 2, 3, 4, 1, 5).reshape(nrb, 32, 64, 4).contiguous()


def from_blocked_x(xb, M):
    nrb = xb.shape[0]
    return xb.view(nrb, 8, 4, 2, 32, 4).permute(0, 4, 1, 2, 3, 5).reshape(nrb * 32, D)[:M].contiguous()


def from_blocked16(buf, M, N):
    """The blocked 16-bit tail of N columns -> row-major [M][N] (as test_gpu_kernels.py states it)."""
    nrb = rows32(M) // 32
    return buf.view(nrb, N // 32, 2, 2, 32, 8).permute(0, 4, 1, 2, 3, 5).reshape(nrb * 32, N)[:M]


def swap_chunks(idx, a=8, b=16):
    """The index map with the 8-column chunks at columns a and b exchanged (a mistake)."""
    out = idx.clone()
    out[:, a:a + 8], out[:, b:b + 8] = idx[:, b:b + 8], idx[:, a:a + 8]
    return out


# ================================================================================================ the float64 model
def layer_norm64(x, dx, a, b, eps, mistakes=(), which=""):
    """(y, dy): the reference's LayerNorm of float64 rows x in float64, and the bound of the fp32 kernel's y (before it is rounded to
    the operand) given |x_kernel - x| <= dx: two-pass mean / centred sum of squares / 1 / (std + eps) / one fma per element."""
    n = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    c = x - mean
    ss = (c * c).sum(-1, keepdim=True)
    std = (ss / (n if which + "_biased_std" in mistakes else n - 1)).sqrt()
    s = (std * std + eps).sqrt() if which + "_eps_in_var" in mistakes else std + eps
    y = a * c / s + b
    dm = dx.mean(-1, keepdim=True) + 2 * gamma(n + 1) * x.abs().mean(-1, keepdim=True)
    dc = dx + dm + 2 * EPS * c.abs()
    ds = (dc * dc).sum(-1, keepdim=True).div(n - 1).sqrt() + 2 * gamma(n + 4) * std + 4 * EPS * s
    # first order in dc with the denominator's own uncertainty; where that is as large as the denominator (bf16 operands behind a
    # d_ff-long product: the worst case grows with K, the error with sqrt(K)) only |c_i| / std <= sqrt(n - 1) is left
    first = torch.where(ds < s, a.abs() * (dc + c.abs() * ds / s) / (s - ds).clamp(min=1e-300), torch.full_like(y, float("inf")))
    dy = torch.minimum(first, a.abs() * (n ** 0.5 + c.abs() / s)) + 8 * EPS * (a * c / s).abs() + 2 * EPS * y.abs()
    return y, dy


def chain_model(x, ctx, w, layout, dff, tail_n, has_next, swish=False, eps=1e-6, mistakes=()):
    """One launch in float64 -> dict(x, ln, tail: (fp64 result, bound, emulation, fp32 accumulation rms term) or None).

    x (M, 256) float32; ctx (M, 256) of the layout's 16-bit type or None; w: float32 wo, bo, a1, b1n, w1, b1, w2, b2, na, nb, wt,
    bt.  ``mistakes`` change the EMULATION only (names from MISTAKES): a stand-in for a kernel that is wrong."""
    bad = set(mistakes)
    dt, u, usub = DTYPES[layout], U_OP[layout], U_SUB[layout]
    rw = lambda t: t.to(dt).double()                       # a weight as the kernel's operand
    rop = lambda t: t.float().to(dt).double()              # an intermediate: fp32 -> operand
    f64 = lambda t: t.double()
    row_rms = lambda t: t.pow(2).mean(-1, keepdim=True).sqrt()
    act = (lambda v: v * torch.sigmoid(v)) if swish else torch.relu
    act_bad = torch.relu if swish else (lambda v: v * torch.sigmoid(v))
    X = f64(x)
    E = X.clone()                                          # the emulation's x
    dX = torch.zeros_like(X)                               # bound of the kernel's fp32 x
    acc2 = torch.zeros_like(X)                             # (fp32 accumulation, random walk)^2
    if ctx is not None:
        C_, Wo, bo = f64(ctx), rw(w["wo"]), f64(w["bo"])
        p = C_ @ Wo.T
        S = C_.abs() @ Wo.abs().T + bo.abs() + X.abs()
        # terms that are exactly 0 add without a rounding: a row of zeros in ctx leaves the two additions x + bo
        k = (C_ != 0).sum(-1, keepdim=True).double() + 2
        X = X + p + bo
        dX = 2 * gamma(k) * S
        acc2 = acc2 + (EPS * (X.abs() + row_rms(p) + bo.abs())) ** 2 * k
        E = (0.0 if "no_residual_attn" in bad else E) + p + (0.0 if "no_bo" in bad else bo)
    if dff:
        a1, b1n, W1, b1, W2, b2 = f64(w["a1"]), f64(w["b1n"]), rw(w["w1"]), f64(w["b1"]), rw(w["w2"]), f64(w["b2"])
        y, dy = layer_norm64(X, dX, a1, b1n, eps)
        e1 = dy + u * (y.abs() + dy) + usub                # |operand - y|
        pre = y @ W1.T + b1
        dpre = e1 @ W1.abs().T + 2 * gamma(D + 1) * ((y.abs() + e1) @ W1.abs().T + b1.abs())
        h = act(pre)
        # (a ReLU whose input is negative beyond its bound gives an exact 0 in the kernel too)
        dh = SWISH_LIP * dpre if swish else torch.where(pre < -dpre, torch.zeros_like(dpre), dpre)
        if swish:                                          # __expf and the reciprocal: a few ulp, growing with |v|
            dh = dh + 2 * (4 * pre.abs() + 16) * EPS * h.abs()
        eh = dh + u * (h.abs() + dh) + usub
        q = h @ W2.T
        S = (h.abs() + eh) @ W2.abs().T + b2.abs() + X.abs() + dX
        X = X + q + b2
        dX = dX + eh @ W2.abs().T + 2 * gamma(dff + 3) * S
        acc2 = acc2 + (EPS * (X.abs() + row_rms(q) + b2.abs())) ** 2 * (dff + 2)
        ye, _ = layer_norm64(E, torch.zeros_like(E), a1, b1n, eps, bad, "ln1")
        he = rop((act_bad if "act_swapped" in bad else act)(rop(ye) @ W1.T + (0.0 if "no_b1" in bad else b1)))
        E = (0.0 if "no_residual_ffn" in bad else E) + he @ W2.T + (0.0 if "no_b2" in bad else b2)
    res = {"x": (X, dX, E.float().double(), acc2.sqrt()), "ln": None, "tail": None}
    if has_next:
        na, nb = f64(w["na"]), f64(w["nb"])
        y, dy = layer_norm64(X, dX, na, nb, eps)
        if "lnn_uses_ln1_vectors" in bad:
            ye, _ = layer_norm64(E, torch.zeros_like(E), f64(w["a1"]), f64(w["b1n"]), eps, bad, "lnn")
        else:
            ye, _ = layer_norm64(E, torch.zeros_like(E), na, nb, eps, bad, "lnn")
        ye = rop(ye)
        half = lambda ref, b_: 0.5 * torch.maximum(out_ulp(ref.abs() + b_, layout), torch.full_like(ref, 2 * usub))
        res["ln"] = (y, dy + half(y, dy), ye, torch.zeros_like(y))
        if tail_n:
            Wt, bt = rw(w["wt"]), f64(w["bt"])
            en = dy + u * (y.abs() + dy) + usub
            t = y @ Wt.T + bt
            S = (y.abs() + en) @ Wt.abs().T + bt.abs()
            dtl = en @ Wt.abs().T + 2 * gamma(D + 1) * S
            te = rop(ye @ Wt.T + (0.0 if "no_bt" in bad else bt))
            res["tail"] = (t, dtl + half(t, dtl), te, EPS * (row_rms(t) + bt.abs()) * (D + 1) ** 0.5)
    return res


# ================================================================================================ cases
def case(name, site, M, rows=None, ctx=None, ldctx=D, dff=0, tail=0, has_next=True, ln_to=None, ln_blk=False, out_blk=False, ldo=None,
         ld_ln=D, store_x=True, xin_blk=False, xout_blk=False, swish=False, adv=False, f8=False):
    """One launch.  M: the rows the host names (the grid); rows: the device-side count (rows_dev) or None; ctx: None / "rm" / "blk";
    ln_to: where LNn(x) goes - None (nowhere: a tail alone, or no next norm), "out" (tail == 0) or "ln_out" (beside the tail)."""
    if ldo is None:
        ldo = tail if tail else D
    return dict(name=name, site=site, M=M, rows=rows, ctx=ctx, ldctx=ldctx, dff=dff, tail=tail, has_next=has_next, ln_to=ln_to,
                ln_blk=ln_blk, out_blk=out_blk, ldo=ldo, ld_ln=ld_ln, store_x=store_x, xin_blk=xin_blk, xout_blk=xout_blk, swish=swish,
                adv=adv, f8=f8)


M_ALL = (1, 31, 32, 33, 127, 128, 129, 257)
M_FEW = (1, 33, 129)


def _cases():
    out = []

    def add(name, site, Ms, adv_M=129, **kw):
        for M in Ms:
            rows = None
            if kw.get("rows") == "dev":  # the device holds the count: the host's M is a capacity that ends in another workgroup
                rows = M
            k = dict(kw, rows=rows)
            out.append(case(f"{name}-M{M}", site, M if rows is None else rows + 131, **k))
        M = adv_M
        k = dict(kw, rows=M if kw.get("rows") == "dev" else None)
        out.append(case(f"{name}-M{M}-adversarial", site, M if k["rows"] is None else M + 131, adv=True, **k))

    # ---- encoder entry (model.hip: run_chain(m->enc_entry ...)): LayerNorm (+ Q|K|V) of layer 0, x row-major and left alone
    add("enc_entry_qkv", "model.hip:233", M_FEW, tail=768, out_blk=True, store_x=False)
    add("enc_entry_ln", "model.hip:231", M_FEW, ln_to="out", ln_blk=True, store_x=False)
    # ---- encoder layer n > 0 (blocked ctx from the attention kernel, x blocked in and out), layer 0 (x row-major in)
    add("enc_layer_qkv", "model.hip:262", M_ALL, ctx="blk", dff=2048, tail=768, out_blk=True, xin_blk=True, xout_blk=True)
    add("enc_layer_ln", "model.hip:260", M_ALL, ctx="blk", dff=2048, ln_to="out", ln_blk=True, xin_blk=True, xout_blk=True)
    add("enc_layer0_qkv", "model.hip:262 (n = 0)", M_FEW, ctx="blk", dff=2048, tail=768, out_blk=True, xout_blk=True)
    # ---- last encoder layer: blocked K|V tail of the decoder side AND row-major enc_h; without decoder-side K|V: enc_h alone
    add("enc_last_kv_ln", "model.hip:256", M_ALL, ctx="blk", dff=2048, tail=1536, out_blk=True, ln_to="ln_out", ld_ln=D, xin_blk=True,
        store_x=False)
    add("enc_last_ln", "model.hip:262 (last)", M_ALL, ctx="blk", dff=2048, ln_to="out", ldo=D + 32, xin_blk=True, store_x=False)
    # ---- decoder side, row count on the device: entry (x row-major, not stored) and the chain between attentions
    add("dec_entry_q", "model.hip:425", M_FEW, rows="dev", tail=256, out_blk=True, store_x=False)
    add("dec_entry_qkv", "model.hip:425", M_FEW, rows="dev", tail=768, out_blk=True, store_x=False)
    add("dec_chain_q", "model.hip:444", M_FEW, rows="dev", ctx="blk", dff=2048, tail=256, out_blk=True, xout_blk=True)
    add("dec_chain_qkv", "model.hip:444", M_FEW, rows="dev", ctx="blk", dff=2048, tail=768, out_blk=True, ldo=768 + 32, xin_blk=True,
        xout_blk=True)
    add("dec_chain_q_rm", "model.hip:444 (row-major)", M_FEW, rows="dev", ctx="rm", ldctx=D + 32, dff=1024, tail=256, ldo=256 + 32)
    add("dec_chain_qkv_rm", "model.hip:444 (row-major)", M_FEW, rows="dev", ctx="rm", ldctx=D + 32, dff=1024, tail=768, ldo=768 + 32)
    add("dec_chain_final", "model.hip:444 (final)", M_FEW, rows="dev", ctx="blk", dff=2048, ln_to="out", ldo=D + 32, xin_blk=True,
        store_x=False)
    add("dec_chain_nocarry", "model.hip:444 (!carry)", M_FEW, rows="dev", ctx="blk", dff=2048, has_next=False, xin_blk=True)
    # ---- conformer layer (sublayers.hip, run_conformer_layer_chain): Swish, row-major ctx and outputs
    add("conf_a", "sublayers.hip:409", M_FEW, dff=2048, tail=768, ldo=768 + 32, xout_blk=True, swish=True)
    add("conf_b", "sublayers.hip:411", M_FEW, ctx="rm", ldctx=D + 32, tail=512, ldo=512 + 32, xin_blk=True, xout_blk=True, swish=True)
    add("conf_c_q", "sublayers.hip:421", M_FEW, ctx="rm", ldctx=D + 32, dff=1024, tail=256, xin_blk=True, xout_blk=True, swish=True)
    add("conf_c_final", "sublayers.hip:420/423", M_FEW, ctx="rm", ldctx=D + 32, dff=1024, ln_to="out", ldo=D + 32, xin_blk=True,
        swish=True)
    # ---- stream lengths of the 8-unit ring
    add("ring_ng0", "NG = 0", M_FEW, ln_to="out", ldo=D + 32)
    add("ring_ng1", "NG = 1", M_FEW, ctx="rm", ldctx=D + 32, has_next=False)
    add("ring_dff128", "d_ff 128", M_FEW, dff=128, ln_to="out", ldo=D + 32)
    add("ring_longest", "d_ff 2048 + tail 1536", M_FEW, ctx="rm", ldctx=D + 32, dff=2048, tail=1536, ldo=1536 + 32, ln_to="ln_out",
        ld_ln=D + 32)
    return out


CASES = _cases()
# the e4m3 feed-forward form as the fp8 engine launches it.  run_enc_layer_fp8 (sublayers.hip) is the UNFUSED path and never
# launches the chain kernel; an fp8 engine with row chains goes down the bf16 engine's path (model.hip), so its chain launches
# read the attention kernel's blocked ctx: that form, with the emulation and tolerance of test_chain_fp8_feed_forward
F8_CASE = case("enc_layer_qkv_f8-M129", "model.hip:262 (fp8 engine)", 129, ctx="blk", dff=512, tail=768, out_blk=True, xin_blk=True,
               xout_blk=True, f8=True)


def weights(dff, tail, seed):
    """Seeded weights as test_chain_bf16 draws them, LayerNorm gains spread over 0.1 .. 4."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    gain = lambda: torch.exp(torch.rand(D, generator=g) * np.log(40.0) + np.log(0.1)).float()
    dff_, tail_ = max(dff, 1), max(tail, 1)
    w = dict(wo=rn(D, D) / 16, bo=0.1 * rn(D), a1=gain(), b1n=0.1 * rn(D), w1=rn(dff_, D) / 16, b1=0.1 * rn(dff_),
             w2=rn(D, dff_) / dff_ ** 0.5, b2=0.1 * rn(D), na=gain(), nb=0.1 * rn(D), wt=rn(tail_, D) / 16, bt=0.1 * rn(tail_))
    return {k: v.contiguous() for k, v in w.items()}


_W = {}


def weights_of(c):
    """One set per (d_ff, tail): the cases of a form share their tensors."""
    key = (c["dff"], c["tail"])
    if key not in _W:
        _W[key] = weights(c["dff"], c["tail"], 1000 + c["dff"] + c["tail"])
    return _W[key]


def inputs(c, layout):
    """(x float32 (rows, 256), ctx 16-bit (rows, 256) or None) of the live rows.  Adversarial cases: a nearly constant row (std
    1e-5 around 2^-7, so eps matters) as the last row, a row with one channel at 1e3, a row of zeros; where the launch has an output
    projection those rows' ctx is 0 and x = row - bo, so that the first LayerNorm still meets them."""
    n = c["M"] if c["rows"] is None else c["rows"]
    g = torch.Generator().manual_seed(sum(map(ord, c["name"])) * 7 + n)
    x = torch.randn(n, D, generator=g) * 2 + 0.3
    ctx = torch.randn(n, D, generator=g).to(DTYPES[layout]) if c["ctx"] else None
    if c["adv"]:
        sub = weights_of(c)["bo"] if c["ctx"] else torch.zeros(D)
        big = torch.randn(D, generator=g)
        big[77] = 1e3
        for r, row in ((n - 1, 2.0 ** -7 + 1e-5 * torch.randn(D, generator=g)), (31, big), (32, torch.zeros(D))):
            x[r] = row - sub
            if ctx is not None:
                ctx[r] = 0
    return x, ctx


_MODEL = {}


def model_of(c, layout):
    """chain_model of the case (computed once per case and layout, shared by every test that needs it)."""
    key = (c["name"], layout)
    if key not in _MODEL:
        x, ctx = inputs(c, layout)
        _MODEL[key] = chain_model(x, ctx, weights_of(c), layout, c["dff"], c["tail"], c["has_next"], c["swish"])
    return _MODEL[key]


# ================================================================================================ buffers of a launch
def buffers(c, layout):
    """Host buffers of the launch, as the kernel reads and writes them: flat tensors x (float32), ctx, out, ln_out (16-bit; None
    where the launch has none).  Rows the launch does not own hold NaN on the input side (rows past the live ones, spare columns)
    and SENTINEL on the output side; every buffer ends with 32 spare rows."""
    dt = DTYPES[layout]
    n = c["M"] if c["rows"] is None else c["rows"]
    cap = rows32(c["M"]) + 32
    x, ctx = inputs(c, layout)
    b = {}
    xb = torch.full((cap * D,), NAN)
    xb[(xblk_index(n) if c["xin_blk"] else rm_index(n, D, D)).reshape(-1)] = x.reshape(-1)
    b["x"] = xb
    b["ctx"] = None
    if ctx is not None:
        cb = torch.full((cap * c["ldctx"],), NAN, dtype=dt)
        cb[(oblk_index(n) if c["ctx"] == "blk" else rm_index(n, D, c["ldctx"])).reshape(-1)] = ctx.reshape(-1)
        b["ctx"] = cb
    has_out = c["tail"] > 0 or c["ln_to"] == "out"
    b["out"] = torch.full((cap * c["ldo"],), SENTINEL, dtype=dt) if has_out else None
    b["ln_out"] = torch.full((cap * c["ld_ln"],), SENTINEL, dtype=dt) if c["ln_to"] == "ln_out" else None
    return b


def places(c):
    """Where the launch's results live: name -> (which buffer, (rows, cols) index of the live elements, index of the elements the
    launch may write without meaning: the rows of the last 32-row block past the live ones in a blocked form)."""
    n = c["M"] if c["rows"] is None else c["rows"]
    pad = lambda index: index(rows32(n))[n:].reshape(-1)
    none = torch.zeros(0, dtype=torch.long)
    p = {}
    if c["store_x"] and (c["ctx"] or c["dff"]):
        p["x"] = ("x", xblk_index(n), pad(xblk_index)) if c["xout_blk"] else ("x", rm_index(n, D, D), none)
    if c["ln_to"]:
        buf, ld = ("out", c["ldo"]) if c["ln_to"] == "out" else ("ln_out", c["ld_ln"])
        p["ln"] = (buf, lnblk_index(n), pad(lnblk_index)) if c["ln_blk"] else (buf, rm_index(n, D, ld), none)
    if c["tail"]:
        if c["out_blk"]:
            p["tail"] = ("out", blk16_index(n, c["tail"], c["ldo"]), pad(lambda r: blk16_index(r, c["tail"], c["ldo"])))
        else:
            p["tail"] = ("out", rm_index(n, c["tail"], c["ldo"]), none)
    return p


def emulate_launch(c, layout, b, mistakes=()):
    """What a launch leaves in the buffers ``b`` (in place), from the emulation: a stand-in for the kernel on the CPU.  ``mistakes``:
    names from MISTAKES.  The rows of a blocked form's last block past the live ones take the value 3 (written without meaning)."""
    bad = set(mistakes)
    assert bad <= set(MISTAKES), bad
    dt = DTYPES[layout]
    n = c["M"] if c["rows"] is None else c["rows"]
    xi = xblk_index(n) if c["xin_blk"] else rm_index(n, D, D)
    if "xin_blk_chunks" in bad and c["xin_blk"]:
        xi = swap_chunks(xi)
    x = b["x"][xi]
    ctx = None
    if c["ctx"]:
        ld = D if "ldctx_ignored" in bad else c["ldctx"]
        ci = oblk_index(n) if c["ctx"] == "blk" else rm_index(n, D, ld)
        if "ctx_blk_chunks" in bad and c["ctx"] == "blk":
            ci = swap_chunks(ci)
        ctx = b["ctx"][ci]
    if "clamp_to_capacity" in bad and n % 32:  # the last live row is computed from the row at the end of the host's M
        x = x.clone()
        x[n - 1] = b["x"][(xblk_index(c["M"]) if c["xin_blk"] else rm_index(c["M"], D, D))[c["M"] - 1]]
    res = chain_model(x, ctx, weights_of(c), layout, c["dff"], c["tail"], c["has_next"], c["swish"], mistakes=bad)
    for name, (buf, idx, padding) in places(c).items():
        val = res[name][2]
        if name == "tail" and "tail_tile_shifted" in bad:  # tile 1 lands in tile 2's place; its own place is not written
            idx = torch.cat([idx[:, :32], idx[:, 64:96], idx[:, 96:]], 1)
            val = torch.cat([val[:, :32], val[:, 32:64], val[:, 96:]], 1)
        blocked = c[{"x": "xout_blk", "ln": "ln_blk", "tail": "out_blk"}[name]]
        which = {"x": "xout_blk_chunks", "ln": "ln_blk_chunks", "tail": "out_blk_chunks"}[name]
        if which in bad and blocked:
            idx = swap_chunks(idx)
        if "store_at_capacity" in bad and n % 32 and not blocked:  # the last live row's values go to the host's row M - 1
            ld = D if name == "x" else (c["ldo"] if buf == "out" else c["ld_ln"])
            idx = idx.clone()
            idx[n - 1] = idx[n - 1] - (n - 1) * ld + (c["M"] - 1) * ld
        b[buf][padding] = 3.0
        b[buf][idx.reshape(-1)] = val.reshape(-1).to(b[buf].dtype)
    return b


class LaunchError(AssertionError):
    """A launch that fails check_launch.  kind: "untouched", "bound" or "ratio"; ratio: the rms ratio of a "ratio" failure."""

    def __init__(self, kind, text, ratio=None):
        super().__init__(text)
        self.kind, self.ratio = kind, ratio


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def check_launch(c, layout, before, after, worst=None):
    """The two checks of the module's docstring on every output of the launch, and: what the launch does not own is untouched bit
    for bit (x of a launch that does not store it; sentinels in spare columns, rows and blocks).  ``worst``: a dict that collects
    (bound ratio, rms ratio) per (layout, site, output)."""
    res = model_of(c, layout)
    pl = places(c)
    for buf in ("x", "out", "ln_out"):
        if before[buf] is None:
            continue
        own = torch.zeros(before[buf].numel(), dtype=torch.bool)
        for name, (b_, idx, padding) in pl.items():
            if b_ == buf:
                own[idx.reshape(-1)] = True
                own[padding] = True
        same = bits(before[buf]) == bits(after[buf])
        if not bool(same[~own].all()):
            where = int((~same & ~own).nonzero()[0])
            raise LaunchError("untouched", f"{layout} {c['name']}: {buf}[{where}] was written and is not the launch's to write "
                              f"({int((~same & ~own).sum())} such elements)")
    for name, (buf, idx, _) in pl.items():
        ref, bound, emu, acc = res[name]
        got = after[buf][idx].double()
        err = (got - ref).abs()
        if not bool((err <= bound).all()):
            badm = ~(err <= bound)
            at = tuple(int(v) for v in badm.nonzero()[0])
            raise LaunchError("bound", f"{layout} {c['name']} {name}: |err| {float(err[at]):.3e} > bound {float(bound[at]):.3e} at "
                              f"(row, column) = {at}; got {float(got[at]):.6g}, fp64 {float(ref[at]):.6g}; {int(badm.sum())} elements "
                              "out of bound")
        rms = lambda t: float(t.pow(2).mean().sqrt())
        yard = (rms(emu - ref) ** 2 + rms(acc) ** 2) ** 0.5
        ratio = rms(got - ref) / yard if yard > 0 else (0.0 if rms(got - ref) == 0 else float("inf"))
        bratio = float((err / bound.clamp(min=1e-300)).max())
        if worst is not None:
            key = (layout, c["name"].split("-M")[0], name)
            old = worst.get(key, (0.0, 0.0))
            worst[key] = (max(old[0], bratio), max(old[1], ratio))
        if not ratio <= RATIO[layout]:
            raise LaunchError("ratio", f"{layout} {c['name']} {name}: rms(result - fp64) {rms(got - ref):.3e} is {ratio:.2f} x the "
                              f"yardstick {yard:.3e} (emulation {rms(emu - ref):.3e}); allowed {RATIO[layout]}", ratio)
