"""A float64 model of one launch of the split-bf16 engine's two own kernels - the d_model-deep projection (csrc/proj_x3.hip,
cn_op_proj_x3_desc) and the fused feed-forward sublayer with its row-chain forms (csrc/fused_x3.hip, cn_op_ffn_x3_act and
cn_op_x3_chain) - with a per-element error bound, the buffers of every launch form and the checks a launch must pass.  Shared by the
kernel test (test_gpu_x3.py), the CPU test that shows the checks catch what a kernel can get wrong (test_x3_model.py) and the
argument test (test_x3_args.py).

The operation is chain_model.py's, on the operands the kernel sees:

    x += Wo . ctx + bo                      if ctx is given                      (PRO)
    x += W2 . act(W1 . LN1(x) + b1) + b2    act: ReLU, or Swish in the plain split form
    y = LNn(x)                              if the next LayerNorm is given
    out = Wt . y + bt (the tail, TAIL) or y itself (xn_out)

and the projection alone, C = [resid + resid_scale *] (A . W^T + bias), is the tail stage by itself with the other stages off.
ctx and A are their hi + lo values.  Split weights are hi + lo as pack_proj_x3 / pack_ffn_x3 split them.  In the mixed form (MIX)
the feed-forward weights are what pack_ffn_mix stores: w = half(w) + l_w, with l_w the e4m3 byte of (w - half(w)) at 2^(lg + 11) and
beside it q_w, the e4m3 byte of w at 2^lg, lg = cn_e4m3_exp(max |W|); the kernel's product of an activation a = h_a + r_a is

    h_a h_w + l_a q_w + q_a l_w             l_a = e4m3(r_a 2^11) 2^-11,  q_a = e4m3(a), both saturating at 448

so that its error against a . w is  (r_a - l_a) q_w + r_a (w - q_w) + (a - q_a) l_w - r_a l_w  (product()).

Two checks per launch (check_launch), no live element exempt from either:

* |out - fp64| <= bound for every live element.  Per product 2 gamma(3 K) sum |a| |w| and the dropped lo . lo term
  (gemm_model.split_product_bound), or in the mixed form the four terms above with each factor bounded - the e4m3 roundoff of l and
  q with their subnormal floor at each scale, r_a r_w, and THE SATURATION TERMS max(|a| - 448, 0) |l_w| and
  max(|r_a| - 448 / 2048, 0) |q_w| for activations beyond the e4m3 range; the split rounding of each stored intermediate
  (LayerNorm output, hidden tile, y); one fp32 rounding per epilogue operation; the first product's bound carried through ReLU /
  Swish (SWISH_LIP) and the second product; x's bound carried through LNn (chain_model.layer_norm64); a split output's halves
  as gemm_model checks them: hi against bf16(v), lo against bf16(v - hi) with the stored hi, hi + lo against v.
* the aggregate check: rms(out - fp64) <= RATIO[family] * sqrt(rms(emulation - fp64)^2 + rms(fp32 random walk)^2).  The
  emulation is the same operation with every operand and intermediate rounding applied (split, or the mixed bytes) and float64
  accumulation.  The yardstick is never a second launch.

And the guards: every input bit for bit as before; NaN in the rows of A / ctx past M and in A's columns 256 .. lda, in resid's
columns N .. ldr and around x; a sentinel in C's columns N .. ldc, in its rows past M and in guard rows in front of and behind
every output; xn_out NaN before the launch and finite in every live element after it, or untouched where the launch has no
xn_out to write (the tail form, no next LayerNorm)."""
import math

import torch

import frontend_model as fm
import gemm_model as gm
from attention_model import EPS, LAYOUTS, from_layout, gamma, out_ulp, to_layout
from chain_model import SWISH_LIP, LaunchError, layer_norm64
from chain_model import weights as chain_weights
from cassnat_asr_public_amd import abi

D = 256
GR = 2  # guard rows in front of and behind every buffer with rows
SENTINEL = 7.0
NAN = float("nan")
LAYOUT = "bf16x3"
assert LAYOUT in LAYOUTS
PRO, TAIL, MIX, SWISH = (abi.CONSTANTS["CN_FFN_X3_" + n] for n in ("PRO", "TAIL", "MIX", "SWISH"))
E4M3_MAX = gm.E4M3_MAX
RANGE_TARGETS = (300, 447, 449, 1000, 30000)

# ---- what the aggregate check allows: rms(out - fp64) / yardstick, per family.  Measured on the MI355X over every case of CASES
# (the table in docs/KERNEL_NOTES.md, "Split-bf16 projections and feed-forward: float64 tests of every launch form"); asserted:
# the measurement times 1.2, rounded up to two digits.
#   family       measured   asserted   closest mistake (test_x3_model.py prints it)
#   proj_f32     0.8354     1.1        489.8 (w_hi_x_lo_dropped)
#   proj_split   0.8937     1.1        389.3 (w_hi_x_lo_dropped)
#   ffn_split    1.0073     1.3        7.43 (ln1_biased_std, a `small` case), 12.7 (w_hi_x_lo_dropped) apart from those
#   ffn_mix      1.0861     1.4        7.39 (ln1_biased_std, a `small` case), 17.0 (mix_act_l_scale_2_10) apart from those
# (out_hi_lo_swapped leaves hi + lo and with it the ratio as they are: the checks of the halves catch it.)  The projection's fp32
# output is below 1 because the yardstick's random-walk term over-estimates the matrix core's fp32 accumulation, the split output
# because a lo half rounds better than its worst case; the feed-forward forms sit at 1.00 but for M = 1 (256 elements: 1.09).
RATIO = {"proj_f32": 1.1, "proj_split": 1.1, "ffn_split": 1.3, "ffn_mix": 1.4}

MISTAKES = ("w_lo_x_hi_dropped", "w_hi_x_lo_dropped", "out_hi_lo_swapped", "lo_plane_offset", "halfwave_groups_not_swapped",
            "chunk_last_tile_skipped", "tail_tile_shifted", "rows_past_M_stored", "last_row_duplicated", "resid_scale_ignored",
            "resid_read_after_store", "no_b1", "no_b2", "no_bo", "no_bt", "relu_before_bias", "swish_as_relu", "ln1_biased_std",
            "lnn_eps_in_var", "lnn_uses_ln1_vectors", "mix_l_q_swapped", "mix_weight_scale_x2", "mix_act_l_scale_2_10",
            "mix_q_not_saturated")


# ================================================================================================ cases
def proj(name, site, M, N, split, resid=None, rs=1.0, lda_pad=0, ldc_pad=0, ldr_pad=0):
    """One projection launch.  resid: None / "sep" / "alias" (C is the residual stream, ldr == ldc)."""
    assert resid in (None, "sep", "alias") and not (split and resid)
    return dict(kind="proj", name=name, site=site, M=M, N=N, split=split, resid=resid, rs=rs, lda=D + lda_pad, ldc=N + ldc_pad,
                ldr=N + (ldc_pad if resid == "alias" else ldr_pad))


def ffn(name, site, M, dff, ctx=False, tail=0, has_next=True, mix=False, swish=False, adv=False, rng=None, small=False):
    """One feed-forward / row-chain launch.  rng: None or (where, target): where = "hidden" (planted b1 entries) or "ln" (scaled
    ln_a) puts a few hidden units or LayerNorm outputs at about `target`.  small: W2 and b2 scaled by 1e-3 and row 5 of x nearly
    constant (std 1e-2 around 2^-7) - the sublayer then leaves that row nearly constant in front of LNn too, where eps against the
    std (and not under the root) is 0.5 % of the result."""
    return dict(kind="ffn", name=name, site=site, M=M, dff=dff, ctx=ctx, tail=tail, has_next=has_next or tail > 0, mix=mix, swish=swish,
                adv=adv, rng=rng, small=small)


def form_bits(c):
    return (PRO if c["ctx"] else 0) | (TAIL if c["tail"] else 0) | (MIX if c["mix"] else 0) | (SWISH if c["swish"] else 0)


def form_name(c, mt=None):
    if c["kind"] == "proj":
        return f"proj MT{(2 if c['M'] >= 4096 else 1) if mt is None else mt} {'split' if c['split'] else 'f32'}"
    b = form_bits(c)
    return "ffn " + ("+".join(n for n, v in (("PRO", PRO), ("TAIL", TAIL), ("MIX", MIX), ("SWISH", SWISH)) if b & v) or "plain")


def family(c):
    if c["kind"] == "proj":
        return "proj_split" if c["split"] else "proj_f32"
    return "ffn_mix" if c["mix"] else "ffn_split"


def _cases():
    out = []
    P = lambda *a, **k: out.append(proj(*a, **k))
    # ---- 32-row workgroups (MT = 1): every ragged edge of M; N from one tile to the widest, fewer tiles than waves, tile counts not
    # divisible by 4, chunk counts 1, 2, 3, 6 and 8; every epilogue; dense and padded strides
    P("M1-N32-f32", "one row, one tile", 1, 32, False)
    P("M31-N64-split", "two tiles", 31, 64, True)
    P("M32-N96-resid", "resid from its own buffer, ldr > N", 32, 96, False, resid="sep", ldr_pad=32)
    P("M33-N128-split-padded", "lda > 256, ldc > N", 33, 128, True, lda_pad=32, ldc_pad=32)
    P("M64-N160-alias-half", "resid aliases C, resid_scale 0.5", 64, 160, False, resid="alias", rs=0.5)
    P("M65-N160-resid-half-padded", "resid_scale 0.5, every stride padded", 65, 160, False, resid="sep", rs=0.5, lda_pad=32, ldc_pad=32,
      ldr_pad=64)
    P("M65-N256-split", "two chunks", 65, 256, True)
    P("M33-N384-split", "three chunks", 33, 384, True, ldc_pad=32)
    P("M65-N768-f32-alias", "six chunks, in place", 65, 768, False, resid="alias")
    P("M33-N1024-f32-padded", "eight chunks, ldc > N", 33, 1024, False, ldc_pad=32)
    P("M64-N1024-split", "eight chunks", 64, 1024, True)
    # ---- the engine's call sites with its own strides (run_linear: lda = d, ldc = the buffer's width)
    P("qkv_proj-M65", "model.hip:237 qkv_proj (ldc = 3 d)", 65, 768, True)
    P("src_q_proj-M33", "model.hip:345 src_q_proj (ldc = d)", 33, 256, True)
    P("out_proj_resid-M65", "sublayers.hip:211 out_proj_resid (x in place)", 65, 256, False, resid="alias")
    P("src_kv_proj-M4095", "sublayers.hip:443 src_kv_proj (ldc = 2 d), MT = 1's last M, 256 workgroups reached", 4095, 512, True)
    # ---- 64-row workgroups (MT = 2, from 4096 rows): full tiles, one live row, a partial second M-tile
    P("M4096-N256-split", "MT 2 full tiles", 4096, 256, True)
    P("M4096-N32-f32", "MT 2 one tile", 4096, 32, False)
    P("M4097-N128-alias", "MT 2 one live row, in place", 4097, 128, False, resid="alias")
    P("out_proj_resid-M4097", "sublayers.hip:211 out_proj_resid, MT 2", 4097, 256, False, resid="alias")
    P("M4127-N64-resid-half-padded", "MT 2 partial second M-tile, resid_scale 0.5", 4127, 64, False, resid="sep", rs=0.5, lda_pad=32,
      ldc_pad=32, ldr_pad=32)
    P("M4127-N256-split-padded", "MT 2 partial second M-tile", 4127, 256, True, lda_pad=32, ldc_pad=32)

    Fq = lambda *a, **k: out.append(ffn(*a, **k))
    for mix in (False, True):
        t = "mix" if mix else "split"
        # ---- the plain form over every ragged edge of M (64-row workgroups) and d_ff (one tile per wave up to sixteen)
        for M, dff, nxt in ((1, 128, True), (31, 256, False), (32, 1024, True), (33, 2048, True), (63, 128, False), (64, 256, True),
                            (65, 2048, True), (65, 1024, False), (129, 128, True)):
            Fq(f"plain-{t}-M{M}-dff{dff}{'' if nxt else '-last'}", "sublayers.hip:78 run_ffn", M, dff, has_next=nxt, mix=mix)
        # ---- output-projection prologue, with and without the next LayerNorm
        Fq(f"pro-{t}-M65-dff256", "PRO", 65, 256, ctx=True, mix=mix)
        Fq(f"pro-{t}-M33-dff128-last", "PRO, no next LayerNorm", 33, 128, ctx=True, has_next=False, mix=mix)
        # ---- Q|K|V tail
        Fq(f"tail-{t}-M65-dff128-t128", "TAIL", 65, 128, tail=128, mix=mix)
        Fq(f"tail-{t}-M1-dff256-t1024", "TAIL", 1, 256, tail=1024, mix=mix)
        # ---- both: the engine's encoder layer
        Fq(f"chain-{t}-M65-dff2048-t768", "sublayers.hip:149 run_x3_chain (Q|K|V)", 65, 2048, ctx=True, tail=768, mix=mix)
        Fq(f"chain-{t}-M129-dff1024-t256", "sublayers.hip:149 run_x3_chain (Q)", 129, 1024, ctx=True, tail=256, mix=mix)
        Fq(f"chain-{t}-M64-dff128-t1024", "PRO + TAIL", 64, 128, ctx=True, tail=1024, mix=mix)
        # ---- adversarial rows
        Fq(f"plain-{t}-M65-dff256-adversarial", "adversarial rows", 65, 256, mix=mix, adv=True)
        Fq(f"chain-{t}-M65-dff256-t256-adversarial", "adversarial rows", 65, 256, ctx=True, tail=256, mix=mix, adv=True)
        # ---- a nearly constant row in front of BOTH LayerNorms
        Fq(f"small-{t}-M65-dff128", "nearly constant row in front of LNn", 65, 128, mix=mix, small=True)
        Fq(f"small-tail-{t}-M33-dff128-t128", "nearly constant row in front of LNn, TAIL", 33, 128, tail=128, mix=mix, small=True)
        # ---- activations around and beyond the e4m3 range of the mixed form; the split form on the same inputs
        for where in ("hidden", "ln"):
            for tg in RANGE_TARGETS:
                Fq(f"range-{where}-{tg}-{t}", f"{where} at about {tg}", 65, 128, mix=mix, rng=(where, tg))
    Fq("swish-M65-dff128", "sublayers.hip:78 run_ffn (conformer AST decoder)", 65, 128, swish=True)
    Fq("swish-M65-dff2048", "sublayers.hip:78 run_ffn (conformer AST decoder)", 65, 2048, swish=True)
    Fq("swish-M31-dff2048-last", "Swish, no next LayerNorm", 31, 2048, swish=True, has_next=False)
    Fq("swish-M129-dff128-adversarial", "Swish, adversarial rows", 129, 128, swish=True, adv=True)
    return out


CASES = _cases()
CHEAP = [c for c in CASES if c["M"] <= 129]  # the cases every mistake is tried on (the wide ones repeat their forms)


def case_id(c):
    return c["name"]


# ================================================================================================ inputs
_W = {}


def weights_of(c):
    """float32 wo, bo, a1, b1n, w1, b1, w2, b2, na, nb, wt, bt (chain_model.weights: LayerNorm gains spread over 0.1 .. 4); one set
    per (d_ff, tail) shared by the cases of a form; a projection's matrix and bias are wt and bt.  Range cases: their own copy with
    the planted entries."""
    if c["kind"] == "proj":
        key = (0, c["N"])
    else:
        key = (c["dff"], c["tail"])
    if key not in _W:
        _W[key] = chain_weights(key[0], key[1], 2000 + key[0] + key[1])
        # bo on a grid of 2^-12: the planted constant row of a row-chain case, x = 2^-7 - bo, then comes back from x + bo exactly
        # constant (std 0).  Off the grid the two roundings leave it a spread of 1e-9, below the fp32 rounding of its own mean, and
        # the row measures that rounding against eps = 1e-6 (docs/KERNEL_NOTES.md has the figure) instead of what eps does.
        _W[key]["bo"] = (_W[key]["bo"] * 4096).round() / 4096
    w = _W[key]
    if c["kind"] == "ffn" and c["small"]:
        w = dict(w, w2=w["w2"] * 1e-3, b2=w["b2"] * 1e-3)
    if c["kind"] == "ffn" and c["rng"]:
        where, tg = c["rng"]
        w = {k: v.clone() for k, v in w.items()}
        if where == "hidden":
            w["b1"][[3, 40, 77, 100]] = float(tg)
        else:  # LN1's output on three channels: its largest magnitude over the rows is the target
            x = _x_of(c).double()
            z = (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + 1e-6)
            for ch in (10, 90, 170):
                w["a1"][ch] = float(tg / z[:, ch].abs().max())
                w["b1n"][ch] = 0.0
    return w


def _gen(c, extra=0):
    return torch.Generator().manual_seed(sum(map(ord, c["name"].replace("-mix", "-split"))) * 7 + c["M"] + extra)


def _x_of(c):
    g = _gen(c)
    x = torch.randn(c["M"], D, generator=g) * 2 + 0.3
    if c["small"]:
        x[5] = 2.0 ** -7 + 1e-2 * torch.randn(D, generator=g)
    if c["adv"]:
        # in front of a LayerNorm: a constant row (std 0: eps decides), a row with one huge element, a row of magnitude 1e-4 beside
        # rows of magnitude 1e3 (what a check against the largest element of the whole output cannot see)
        x[c["M"] - 1] = 2.0 ** -7
        x[31, :] = torch.randn(D, generator=g)
        x[31, 77] = 1e3
        x[32] = 1e-4 * torch.randn(D, generator=g)
        x[33] = 1e3 * torch.randn(D, generator=g)
        x[0] = 1e3 * torch.randn(D, generator=g)
    return x


def inputs(c):
    """proj: A float32 (M, 256) and resid (M, N) or None; ffn: x float32 (M, 256) and ctx float32 (M, 256) or None.  (The mixed and
    the split case of a pair draw the same values.)  In an adversarial row-chain case the planted rows' ctx is 0 and x = row - bo,
    so that the first LayerNorm still meets them."""
    g = _gen(c, 1)
    if c["kind"] == "proj":
        A = torch.randn(c["M"], D, generator=g)
        resid = torch.randn(c["M"], c["N"], generator=g) * 2 if c["resid"] else None
        return A, resid
    x = _x_of(c)
    ctx = torch.randn(c["M"], D, generator=g) if c["ctx"] else None
    if c["adv"] and ctx is not None:
        for r in (c["M"] - 1, 31, 32, 33, 0):
            ctx[r] = 0
            x[r] = x[r] - weights_of(c)["bo"]
    return x, ctx


# ================================================================================================ buffers of a launch
def split_units(n_cols):
    """Unit (bf16) columns of the hi and the lo halves of elements 0 .. n_cols - 1 of a split-bf16 row (cn_split_off)."""
    n = torch.arange(n_cols)
    hi = (n >> 5) * 64 + (n & 31)
    return hi, hi + 32


def _rows(M, ld_units, dtype, fill):
    return torch.full((GR + M + GR, ld_units), fill, dtype=torch.float32).to(dtype)


def _put_split(buf, M, vals32):
    packed, _ = to_layout(vals32, LAYOUT, device="cpu")
    buf[GR:GR + M, :packed.shape[1]] = packed


def buffers(c):
    """Host tensors of the launch as the kernel reads and writes them, each with GR guard rows in front and behind (the rows behind
    are the rows past M).  NaN fills what the launch must not read, SENTINEL what it must not write; vectors and host matrices as
    they are (checked bit for bit afterwards)."""
    w = weights_of(c)
    M = c["M"]
    b = {}
    if c["kind"] == "proj":
        A, resid = inputs(c)
        b["A"] = _rows(M, 2 * c["lda"], torch.bfloat16, NAN)
        _put_split(b["A"], M, A)
        b["wt"], b["bt"] = w["wt"], w["bt"]
        if c["split"]:
            b["C"] = _rows(M, 2 * c["ldc"], torch.bfloat16, SENTINEL)
        elif c["resid"] == "alias":
            b["C"] = _rows(M, c["ldc"], torch.float32, NAN)
            b["C"][GR:GR + M, :c["N"]] = resid
        else:
            b["C"] = _rows(M, c["ldc"], torch.float32, SENTINEL)
        if c["resid"] == "sep":
            b["resid"] = _rows(M, c["ldr"], torch.float32, NAN)
            b["resid"][GR:GR + M, :c["N"]] = resid
        return b
    x, ctx = inputs(c)
    b["x"] = _rows(M, D, torch.float32, NAN)
    b["x"][GR:GR + M] = x
    if ctx is not None:
        b["ctx"] = _rows(M, 2 * D, torch.bfloat16, NAN)
        _put_split(b["ctx"], M, ctx)
    b["xn"] = _rows(M, 2 * D, torch.bfloat16, SENTINEL)
    b["xn"][GR:GR + M] = NAN
    if c["tail"]:
        b["tail"] = _rows(M, 2 * c["tail"], torch.bfloat16, SENTINEL)
    for k in ("wo", "bo", "a1", "b1n", "w1", "b1", "w2", "b2", "na", "nb", "wt", "bt"):
        b[k] = w[k]
    return b


def read_split(buf, M, n_cols):
    hi, lo = split_units(n_cols)
    live = buf[GR:GR + M]
    return live[:, hi].double(), live[:, lo].double()


# ================================================================================================ operands as the kernel sees them
def split_parts(t):
    """float tensor -> (hi, lo) float64 as the host packers and cn_split4 split it."""
    return fm.split16(t.double(), "bf16")


def mix_weight_parts(w):
    """pack_ffn_mix: (h, l, q, lg) of a float32 matrix - half, the e4m3 byte of the remainder at 2^(lg + 11), the e4m3 byte of the
    value at 2^lg."""
    lg = fm.e4m3_exp(float(w.abs().max()))
    h = fm.r16(w.double(), "fp16")
    r = (w.float() - h.float()).double()
    l = fm.e4m3_val(fm.e4m3_bits(r * 2.0 ** (lg + 11))) / 2.0 ** (lg + 11)
    q = fm.e4m3_val(fm.e4m3_bits(w.double() * 2.0 ** lg)) / 2.0 ** lg
    return h, l, q, lg


def mix_act_parts(v, saturate=True):
    """The kernel's three operands of an fp32 activation: half, l = e4m3((v - h) 2^11), q = e4m3(v), saturating (frontend_model's
    byte model at MIX_LG_AL, MIX_LG_AQ).  saturate=False: q converted without the clamp (a mistake: NaN past the range)."""
    v32 = v.float()
    h = fm.r16(v32.double(), "fp16")
    sl, sq = 2.0 ** fm.MIX_LG_AL, 2.0 ** fm.MIX_LG_AQ
    l = fm.e4m3_val(fm.e4m3_bits((v32 - h.float()).double() * sl)) / sl
    if saturate:
        q = fm.e4m3_val(fm.e4m3_bits(v32.double() * sq)) / sq
    else:
        q = (v32 * sq).to(torch.float8_e4m3fn).double() / sq
    return h, l, q


class Weight:
    """A matrix as a product sees it: .w (float64, the value the model multiplies by) and the parts the emulation multiplies by."""

    def __init__(self, w32, mix):
        self.mix = mix
        if mix:
            self.h, self.l, self.q, self.lg = mix_weight_parts(w32)
            self.w = self.h + self.l
        else:
            self.hi, self.lo = split_parts(w32)
            self.w = self.hi + self.lo


def product(a, da, W, K, stored, bad=(), emu_a=None):
    """(p, dp, e): p = a . W.w^T in float64; dp bounds |the kernel's fp32 accumulator - p| given that the kernel's fp32 activation is
    within da of a; e = the emulation's product of its own activations emu_a (float64 of fp32 values), with the operand roundings.
    stored: the activation is an fp32 intermediate the kernel rounds (split, or the mixed bytes); False: an operand that is hi + lo
    already (ctx, A)."""
    absW = W.w.abs()
    p = a @ W.w.T
    ab = a.abs() + da
    if not W.mix:
        e_a = da + (out_ulp(ab, LAYOUT) if stored else 0.0)  # |the kernel's hi + lo - a|
        S = (a.abs() + e_a) @ absW.T
        dp = e_a @ absW.T + gm.split_product_bound(S, K)
        ah, al = split_parts(emu_a.float()) if stored else split_parts(emu_a)
        e = ah @ W.hi.T
        if "w_lo_x_hi_dropped" not in bad:
            e = e + ah @ W.lo.T
        if "w_hi_x_lo_dropped" not in bad:
            e = e + al @ W.hi.T
        return p, dp, e
    assert stored
    sl = 2.0 ** fm.MIX_LG_AL
    rb = 0.5 * fm.ulp(ab, "fp16")                                     # |r_a| = |a - half(a)|
    err_l = 0.5 * fm.ulp((rb * sl).clamp(max=E4M3_MAX), "e4m3") / sl + (rb - E4M3_MAX / sl).clamp(min=0)   # |r_a - l_a|
    err_q = 0.5 * fm.ulp(ab.clamp(max=E4M3_MAX), "e4m3") + (ab - E4M3_MAX).clamp(min=0)                    # |a - q_a|
    dp = (da @ absW.T + err_l @ W.q.abs().T + rb @ (W.w - W.q).abs().T + err_q @ W.l.abs().T + rb @ W.l.abs().T
          + 2 * gamma(3 * K) * (ab @ absW.T)
          + gm.E4M3_ACC * (rb @ W.q.abs().T + ab.clamp(max=E4M3_MAX) @ W.l.abs().T))   # the e4m3 MFMA's own summation of the cross terms
    h, l, q = mix_act_parts(emu_a, saturate="mix_q_not_saturated" not in bad)
    if "mix_l_q_swapped" in bad:      # the activation's two bytes in each other's k-block, each read at the other's scale
        l, q = q / sl, l * sl
    t_lq, t_ql = l @ W.q.T, q @ W.l.T
    if "mix_act_l_scale_2_10" in bad:
        t_lq = 2 * t_lq
    if "mix_weight_scale_x2" in bad:
        t_lq, t_ql = 2 * t_lq, 2 * t_ql
    return p, dp, h @ W.h.T + t_lq + t_ql


def step(v, dv):
    """One fp32 rounding of an operation's result v whose inputs carry dv."""
    return dv + EPS * (v.abs() + dv)


def row_rms(t):
    return t.pow(2).mean(-1, keepdim=True).sqrt()


def x3_model(c, ops, mistakes=()):
    """One launch in float64 from the operand values ``ops`` (operands()) -> output name -> dict(ref, dv, emu, acc, kind): the fp64
    result, the bound of the kernel's fp32 value in front of the output's rounding, the emulation's value in front of that rounding
    (``mistakes`` change it and nothing else), the random-walk term, "f32" or "split"."""
    bad = set(mistakes)
    assert bad <= set(MISTAKES), bad
    w = weights_of(c)
    f64 = lambda t: t.double()
    eps = 1e-6
    if c["kind"] == "proj":
        Wt, bt = Weight(w["wt"], False), f64(w["bt"])
        A = ops["A"]
        p, dp, e = product(A, torch.zeros_like(A), Wt, D, False, bad, A)
        v = p + bt
        dv = step(v, dp)
        acc = EPS * math.sqrt(D) * (p.abs() + row_rms(p) + bt.abs())
        e = e + (0.0 if "no_bt" in bad else bt)
        if c["resid"]:
            rs = c["rs"]
            v = rs * v
            dv = step(v, dv * abs(rs))
            v = ops["resid"] + v
            dv = step(v, dv)
            acc = acc * abs(rs)
            scaled = (1.0 if "resid_scale_ignored" in bad else rs) * e
            e = ops["resid"] + scaled
            if "resid_read_after_store" in bad and c["resid"] == "alias":
                e = e + scaled
        return {"C": dict(ref=v, dv=dv, emu=e, acc=acc, kind="split" if c["split"] else "f32")}
    mix = c["mix"]
    X = ops["x"]
    E = X.clone()
    dX = torch.zeros_like(X)
    acc2 = torch.zeros_like(X)
    if c["ctx"]:
        Wo, bo = Weight(w["wo"], False), f64(w["bo"])
        C_ = ops["ctx"]
        p, dp, e = product(C_, torch.zeros_like(C_), Wo, D, False, bad, C_)
        v = p + bo
        dv = step(v, dp)
        X = X + v
        dX = step(X, dv + EPS * v.abs())                   # (resid_scale 1: the multiplication is exact)
        acc2 = acc2 + (EPS * (X.abs() + row_rms(p) + bo.abs())) ** 2 * (D + 2)
        E = (E + (e + (0.0 if "no_bo" in bad else bo)).float().double()).float().double()
    a1, b1n, b1, b2 = f64(w["a1"]), f64(w["b1n"]), f64(w["b1"]), f64(w["b2"])
    W1, W2 = Weight(w["w1"], mix), Weight(w["w2"], mix)
    dff = c["dff"]
    y, dy = layer_norm64(X, dX, a1, b1n, eps)
    ye, _ = layer_norm64(E, torch.zeros_like(E), a1, b1n, eps, bad, "ln1")
    p1, dp1, e1 = product(y, dy, W1, D, True, bad, ye)
    pre = p1 + b1
    dpre = step(pre, dp1)
    swish = lambda t: t * torch.sigmoid(t)
    if c["swish"]:
        h = swish(pre)
        dh = SWISH_LIP * dpre + 2 * (4 * pre.abs() + 16) * EPS * h.abs()   # (chain_model: __expf and the reciprocal)
    else:
        h = torch.relu(pre)
        dh = torch.where(pre < -dpre, torch.zeros_like(dpre), dpre)        # negative beyond its bound: an exact 0 in the kernel too
    if "relu_before_bias" in bad:
        he = torch.relu(e1) + b1
    else:
        pe = e1 + (0.0 if "no_b1" in bad else b1)
        he = torch.relu(pe) if (not c["swish"] or "swish_as_relu" in bad) else swish(pe)
    p2, dp2, e2 = product(h, dh, W2, dff, True, bad, he.float().double())
    # the four waves' partial sums, x and b2: six more additions
    Sx = X.abs() + dX + p2.abs() + dp2 + b2.abs()
    X = X + p2 + b2
    dX = dX + dp2 + 6 * EPS * Sx
    acc2 = acc2 + (EPS * (X.abs() + row_rms(p2) + b2.abs())) ** 2 * (dff + 2)
    E = E + e2 + (0.0 if "no_b2" in bad else b2)
    res = {"x": dict(ref=X, dv=dX, emu=E, acc=acc2.sqrt(), kind="f32")}
    if c["has_next"]:
        na, nb = f64(w["na"]), f64(w["nb"])
        E32 = E.float().double()
        y, dy = layer_norm64(X, dX, na, nb, eps)
        if "lnn_uses_ln1_vectors" in bad:
            ye, _ = layer_norm64(E32, torch.zeros_like(E), a1, b1n, eps, bad, "lnn")
        else:
            ye, _ = layer_norm64(E32, torch.zeros_like(E), na, nb, eps, bad, "lnn")
        if c["tail"]:
            Wt, bt = Weight(w["wt"], False), f64(w["bt"])
            pt, dpt, et = product(y, dy, Wt, D, True, bad, ye)
            t = pt + bt
            res["tail"] = dict(ref=t, dv=step(t, dpt), emu=et + (0.0 if "no_bt" in bad else bt),
                               acc=EPS * math.sqrt(D) * (pt.abs() + row_rms(pt) + bt.abs()), kind="split")
        else:
            res["xn"] = dict(ref=y, dv=dy, emu=ye, acc=torch.zeros_like(y), kind="split")
    return res


def operands(c, b):
    """The float64 values the launch reads from the buffers ``b``."""
    M = c["M"]
    if c["kind"] == "proj":
        o = {"A": from_layout(b["A"][GR:GR + M, :2 * D], LAYOUT)}
        if c["resid"]:
            o["resid"] = (b["C"] if c["resid"] == "alias" else b["resid"])[GR:GR + M, :c["N"]].double()
        return o
    o = {"x": b["x"][GR:GR + M].double()}
    if c["ctx"]:
        o["ctx"] = from_layout(b["ctx"][GR:GR + M], LAYOUT)
    return o


_MODEL = {}


def model_of(c):
    """x3_model of the case's own buffers (computed once per case, shared by every test that needs it)."""
    if c["name"] not in _MODEL:
        _MODEL[c["name"]] = x3_model(c, operands(c, buffers(c)))
    return _MODEL[c["name"]]


# ================================================================================================ a launch on the CPU
def outputs(c):
    """output name -> (buffer name, columns)."""
    if c["kind"] == "proj":
        return {"C": ("C", c["N"])}
    o = {"x": ("x", D)}
    if c["tail"]:
        o["tail"] = ("tail", c["tail"])
    elif c["has_next"]:
        o["xn"] = ("xn", D)
    return o


def applies(mistake, c):
    """Whether a mistake changes anything in the case."""
    k, f = c["kind"], c["kind"] == "ffn"
    # (a range case's planted activations carry roundings larger than what a small term adds: those mistakes are tried elsewhere)
    plain = f and c["rng"] is None
    split_out = (k == "proj" and c["split"]) or (f and c["has_next"])
    ncols = c["N"] if k == "proj" else (c["tail"] if c["tail"] else D)
    return {
        "w_lo_x_hi_dropped": k == "proj" or not c["mix"] or c["ctx"] or c["tail"] > 0,
        "w_hi_x_lo_dropped": k == "proj" or not c["mix"] or c["ctx"] or c["tail"] > 0,
        "out_hi_lo_swapped": split_out, "lo_plane_offset": split_out, "halfwave_groups_not_swapped": split_out,
        "chunk_last_tile_skipped": k == "proj" or c.get("tail", 0) > 0,
        "tail_tile_shifted": (k == "proj" or c.get("tail", 0) > 0) and ncols >= 96 and split_out,
        "rows_past_M_stored": True, "last_row_duplicated": c["M"] >= 2 and not c.get("adv") and not c.get("rng"),
        "resid_scale_ignored": k == "proj" and c["resid"] is not None and c["rs"] != 1.0,
        "resid_read_after_store": k == "proj" and c["resid"] == "alias",
        "no_b1": plain, "no_b2": plain, "no_bo": f and c["ctx"], "no_bt": k == "proj" or c.get("tail", 0) > 0,
        "relu_before_bias": plain and not c["swish"], "swish_as_relu": f and c["swish"],
        # (eps under the root instead of beside the std moves a row of std 2 by 5e-7 of itself, below the split output's step: the
        # mistake shows where a row in front of LNn is nearly constant)
        "ln1_biased_std": plain, "lnn_eps_in_var": f and c["small"], "lnn_uses_ln1_vectors": f and c["has_next"],
        # (in a `small` case the sublayer adds a thousandth of the residual stream, and a cross term's mistake shows a thousandth as well)
        "mix_l_q_swapped": plain and c["mix"] and not c["small"], "mix_weight_scale_x2": plain and c["mix"] and not c["small"],
        "mix_act_l_scale_2_10": plain and c["mix"] and not c["small"],
        "mix_q_not_saturated": f and c["mix"] and c["rng"] is not None and c["rng"][1] >= 1000,
    }[mistake]


def emulate_launch(c, b, mistakes=()):
    """What a launch leaves in the buffers ``b`` (in place), from the emulation: a stand-in for the kernel on the CPU."""
    bad = set(mistakes)
    assert bad <= set(MISTAKES), bad
    res = x3_model(c, operands(c, b), bad) if bad else model_of(c)
    M = c["M"]
    for name, (buf, ncols) in outputs(c).items():
        r = res[name]
        E = r["emu"]
        rows = M
        if "last_row_duplicated" in bad and M >= 2:
            E = torch.cat([E[:-1], E[-2:-1]], 0)
        if "rows_past_M_stored" in bad:  # the clamped source row M - 1 once more, stored at row M
            E, rows = torch.cat([E, E[-1:]], 0), M + 1
        cols = torch.arange(ncols)
        src = cols.clone()
        keep = torch.ones(ncols, dtype=torch.bool)
        tiled = name in ("C", "tail")
        if "chunk_last_tile_skipped" in bad and tiled:
            keep[ncols - 32:] = False
        if "tail_tile_shifted" in bad and tiled and ncols >= 96 and r["kind"] == "split":  # tile 1 lands in tile 2's place
            src[64:96] = cols[32:64]
            keep[32:64] = False
        live = b[buf][GR:GR + rows]
        if r["kind"] == "f32":
            live[:, cols[keep]] = E[:, src[keep]].float()
            continue
        hi, lo = gm.round_out(E, "split")
        if "halfwave_groups_not_swapped" in bad:
            g = src.clone()
            t = cols & 31
            g[(t >= 8) & (t < 16)] += 8
            g[(t >= 16) & (t < 24)] -= 8
            src = g
        hu, lu = split_units(ncols)
        if "out_hi_lo_swapped" in bad:
            hu, lu = lu, hu
        if "lo_plane_offset" in bad:   # the lo halves one group further (into the next row at the end of a row)
            flat = b[buf].view(-1)
            base = (torch.arange(rows) + GR)[:, None] * b[buf].shape[1]
            live[:, hu[keep]] = hi[:, src[keep]]
            flat[(base + lu[keep][None, :] + 64).reshape(-1)] = lo[:, src[keep]].reshape(-1)
            continue
        live[:, hu[keep]] = hi[:, src[keep]]
        live[:, lu[keep]] = lo[:, src[keep]]
    return b


# ================================================================================================ the checks
def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def rms(t):
    return float(t.pow(2).mean().sqrt())


def check_launch(c, before, after, worst=None, enforce=True):
    """The checks of the module's docstring.  ``worst``: a dict that receives output name -> (worst |err| / bound, rms ratio, rms of
    the error).  enforce=False: measure only (the guards still raise)."""
    M = c["M"]
    outs = outputs(c)
    for name, t in before.items():
        same = bits(t) == bits(after[name])
        for oname, (buf, ncols) in outs.items():
            if buf == name:
                kind = model_of(c)[oname]["kind"]
                live = same[GR:GR + M]
                if kind == "f32":
                    live[:, :ncols] = True
                else:
                    hu, lu = split_units(ncols)
                    live[:, hu] = True
                    live[:, lu] = True
        if not bool(same.all()):
            at = tuple(int(v) for v in (~same).nonzero()[0])
            raise LaunchError("untouched", f"{c['name']}: {name}{list(at)} (buffer row - {GR}, unit) was written and is not the launch's "
                              f"to write ({int((~same).sum())} such units)")
    res = model_of(c)
    fam = family(c)
    for oname, (buf, ncols) in outs.items():
        r = res[oname]
        ref, dv = r["ref"], r["dv"]

        def bound_check(what, err, bound, got, want):
            okay = err <= bound
            if enforce and not bool(okay.all()):
                at = tuple(int(v) for v in (~okay).nonzero()[0])
                raise LaunchError("bound", f"{c['name']} {oname} {what}: |err| {float(err[at]):.3e} > bound {float(bound[at]):.3e} at "
                                  f"(row, column) = {at}; got {float(got[at]):.6g}, fp64 {float(want[at]):.6g}; {int((~okay).sum())} "
                                  "elements out of bound")
            q = err / bound.clamp(min=1e-300)
            return float(torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q).max())

        if r["kind"] == "f32":
            got = after[buf][GR:GR + M, :ncols].double()
            bratio = bound_check("", (got - ref).abs(), dv, got, ref)
            emu = r["emu"].float().double()
        else:
            got_hi, got_lo = read_split(after[buf], M, ncols)
            got = got_hi + got_lo
            if buf == "xn" and not bool(torch.isfinite(got).all()):
                raise LaunchError("bound", f"{c['name']}: xn_out has {int((~torch.isfinite(got)).sum())} live elements that are not finite")
            bratio = bound_check("hi half", (got_hi - ref).abs(), dv + 0.5 * out_ulp(ref.abs() + dv, "bf16"), got_hi, ref)
            rest = ref - got_hi  # what the lo half has to hold, given the hi half that was stored
            bratio = max(bratio, bound_check("lo half", (got_lo - rest).abs(), dv + 0.5 * out_ulp(rest.abs() + dv, "bf16"), got_lo, rest))
            bratio = max(bratio, bound_check("hi + lo", (got - ref).abs(), dv + out_ulp(ref.abs() + dv, LAYOUT), got, ref))
            # and, whatever the bound: lo = bf16(v - bf16(v)) is at most half a step of the hi half that is stored beside it
            bound_check("lo half against the stored hi half", got_lo.abs(), 0.5 * (1 + 2.0 ** -8) * out_ulp(got_hi.abs(), "bf16") + 1e-37,
                        got_lo, got_hi)
            emu = gm.emu_value(r["emu"], "split")
        yard = math.sqrt(rms(emu - ref) ** 2 + rms(r["acc"]) ** 2)
        dev = rms(got - ref)
        ratio = dev / yard if yard > 0 else (0.0 if dev == 0 else float("inf"))
        if math.isnan(ratio):
            ratio = float("inf")
        if worst is not None:
            worst[oname] = (bratio, ratio, dev)
        if enforce and not ratio <= RATIO[fam]:
            raise LaunchError("ratio", f"{c['name']} {oname}: rms(result - fp64) {dev:.3e} is {ratio:.3f} x the yardstick {yard:.3e} "
                              f"(emulation {rms(emu - ref):.3e}); allowed {RATIO[fam]} ({fam})", ratio)
