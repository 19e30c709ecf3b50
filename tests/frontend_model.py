"""Float64 models of the subsampling front end (csrc/conv1.hip, conv2.hip, gemm.hip), per-element error bounds, the buffers of
every launch form the engine uses, and the checks a launch must pass.  Shared by the kernel test (test_gpu_frontend.py), the CPU
test that shows what the checks catch (test_frontend_model.py) and the argument test (test_frontend_args.py).

The operations (the reference's Conv2dSubsampling, src/models/modules/embedding.py:102-119):

    conv1   img[b][t1][f1][c] = relu(b1[c] + sum_{kh,kw} x[b][2 t1 - 1 + kh][2 f1 - 1 + kw] w1[c][kh][kw])      Conv2d(1, C, 3, 2, 1)
    conv2   out[(b,t2,f2)][co] = relu(b2[co] + sum_{kh,kw,ci} img[b][2 t2 - 1 + kh][2 f2 - 1 + kw][ci] w2[co][kh][kw][ci])
    linear  y[m][n] = (sum_k a[m][k] w[n][k] + b[n]) * scale + pe[m % pe_period][n]         linear_out, x sqrt(d), + PE rows

zero outside the image.  The merged-pass rule (csrc/kernels.h, UttMeta): utterance b of a merged pass belongs to a batch of
frames[b] <= T frames; frames at or past frames[b] read as zero and image rows at or past (frames[b] - 1) / 2 + 1 are zeros.

Checks per launch (conv1_check / rows_check, driven by run_case):

* |out - fp64| <= bound on every live element.  conv1 rounds nothing but its sums and its output: gamma(10) sum |x||w| for the
  fp32 FMA chain; the matrix-core forms split x, w and the bias into hi + lo 16-bit halves and drop lo . lo (3 u^2 sum |x||w|, an
  absolute term where the half-precision lo half is subnormal) and accumulate 3 x 10 terms in the MFMA adder (factor 2).  conv2
  and linear are given their operands as bytes: the model multiplies what those bytes hold, so only the accumulation
  (2 gamma(K + 1) sum |a||w|) and, in the split forms, the dropped lo . lo products remain.  Half an output step of bf16 / fp16 /
  e4m3 / split-bf16 is added where the output is rounded.  An output whose pre-activation is negative beyond its bound is an
  exact zero.  MIX: the model of the arithmetic is the three-term product h_a h_w + l_a q_w + q_a l_w on the planes' bytes.
* the aggregate check: RMS(out - fp64) over the live elements within RATIO of sqrt(rms(emulation - fp64)^2 + rms(acc)^2), the
  emulation being the same operation with the stage's roundings applied and float64 sums, acc a random-walk estimate of the fp32
  accumulation, EPS sqrt(K) (|sum| + sqrt(sum of squared products)).  Never a second launch.
* exactness: border cells and rows past an utterance's own batch are bit-zero; under halo mode 2 the border keeps the caller's
  bytes; expand_meta's records are equal; hi is the 16-bit rounding of hi + lo in every split form (|lo| <= ulp(hi) / 2).
* guards: NaN in every frame at or past frames[b], in spare lda columns, in rows past M and around every input buffer; NaN bytes
  in every image cell before a halo 0 / 1 launch; a sentinel in output rows past M and around every output buffer.
"""
import math

import numpy as np
import torch
import torch.nn.functional as Fn

from attention_model import EPS, LAYOUTS, gamma

LIBS = [n for n in ("bf16", "fp16") if n in LAYOUTS]
OP16 = {"bf16": torch.bfloat16, "fp16": torch.float16}
MANT = {"bf16": (7, -126), "fp16": (10, -14), "e4m3": (3, -6)}  # (explicit mantissa bits, smallest normal exponent)
GUARD = 4096         # bytes of guard in front of and behind every device buffer
SENT = 0x5A          # the byte a launch must leave alone
MIX_LG_AL, MIX_LG_AQ = 11, 0

# What the aggregate check allows: RMS(out - fp64) / yardstick, per library and kind of output.  Measured on the MI355X over every
# case of CASES (the table in docs/KERNEL_NOTES.md, "Subsampling front end: float64 tests of every launch form").
# "rounded": the output is rounded to bf16 / fp16 / e4m3 / split-bf16, and that rounding IS the error: 0.26 .. 1.000 on every
#   form of both libraries (below 1 where a split output's lo half rounds better than its worst case, or the MIX l byte does).
#   1.1 as in chain_model.RATIO: a tenth above an emulation the kernels meet to the third decimal.
# "f32": nothing is rounded but the sums, the yardstick is the random-walk ESTIMATE of fp32 accumulation, not an emulation:
#   0.05 .. 0.16 for the fp32 FMA chain and the 16-bit and fp32 MFMA sums (which carry more bits inside a block than the
#   estimate assumes), 0.79 for split-bf16 operands, 1.29 .. 1.36 for linear_out's e4m3 form, whose block-scaled MFMA sums 5120
#   products: 1.7 leaves a factor 1.25 above that measurement.  The half-precision library has no e4m3 form: 0.07 at most, 1.1.
# No listed mistake comes near either figure: each one that the exactness checks and guards do not catch breaks the per-element
# bound, and moves this ratio to 90 at the least (test_frontend_model.py::test_mistake_is_caught prints and asserts it).
RATIO = {"bf16": {"rounded": 1.1, "f32": 1.7}, "fp16": {"rounded": 1.1, "f32": 1.1}}

MISTAKES = ("tap_dropped_top", "tap_dropped_bottom", "tap_dropped_left", "tap_dropped_right", "taps_transposed", "halo_cell_nonzero",
            "border_rewritten_halo2", "past_own_unwritten_halo2", "frames_past_read", "t1_own_from_T", "record_of_wrong_batch",
            "flush_at_previous_block", "rows_past_M_stored", "row_split_T1_for_T2", "hi_lo_swapped", "mix_l_q_swapped",
            "e4m3_scale_off_by_one", "bias_missing", "relu_missing", "pe_row_div", "lda_ignored")


def sub(n):
    return (n - 1) // 2 + 1


# ================================================================================================ number formats
def ulp(v, fmt):
    """One step of format ``fmt`` at |v| (float64 tensor)."""
    m, emin = MANT[fmt]
    e = torch.floor(torch.log2(v.abs().clamp(min=1e-300))).clamp(min=emin)
    return torch.exp2(e - m)


def r16(t, layout):
    """float64 -> fp32 -> the library's 16-bit operand -> float64."""
    return t.float().to(OP16[layout]).double()


def bits16(t, layout):
    return t.float().to(OP16[layout]).view(torch.int16).numpy()


def val16(a, layout):
    return torch.from_numpy(np.ascontiguousarray(a)).view(OP16[layout]).double()


def e4m3_bits(t):
    """float64 -> fp32 -> saturating e4m3fn byte (round to nearest even, as v_cvt_pk_fp8_f32 of a clamped value)."""
    return t.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def e4m3_val(a):
    return torch.from_numpy(np.ascontiguousarray(a)).view(torch.float8_e4m3fn).double()


def e4m3_exp(mx):
    """cn_e4m3_exp: the largest lg with mx 2^lg <= 448 (0 for an all-zero tensor)."""
    if not mx > 0:
        return 0
    lg = math.floor(math.log2(448.0 / mx))
    while mx * 2.0 ** (lg + 1) <= 448.0:
        lg += 1
    while mx * 2.0 ** lg > 448.0:
        lg -= 1
    return lg


def split16(t, layout):
    """(hi, lo): hi = r16(t), lo = r16(t - hi)."""
    hi = r16(t, layout)
    return hi, r16(t - hi, layout)


# ================================================================================================ layouts of images and rows
# An image is [B][H][W][C] cells (H, W with the border where there is one).  raw(): the planes of a byte buffer as integer arrays of
# that shape (views of the buffer: writing them writes the buffer); values(): the planes as float64.
IMG_BYTES = {"f32": 4, "16": 2, "x3": 4, "planes": 4, "mix": 4, "e4m3": 1}


def raw(buf, fmt, shape):
    """buf: uint8 ndarray of prod(shape) * IMG_BYTES[fmt] bytes.  Plane name -> integer view of shape ``shape``."""
    n = int(np.prod(shape))
    C = shape[-1]
    if fmt == "f32":
        return {"v": buf.view(np.int32).reshape(shape)}
    if fmt == "16":
        return {"v": buf.view(np.int16).reshape(shape)}
    if fmt == "e4m3":
        return {"v": buf.reshape(shape)}
    if fmt == "x3":  # split-bf16 rows: per group of 32 channels 32 hi halves, then 32 lo halves (cn_split_off)
        g = buf.view(np.int16).reshape(tuple(shape[:-1]) + (C // 32, 2, 32))
        return {"hi": g[..., 0, :], "lo": g[..., 1, :]}  # (strided views of shape [..., C / 32, 32]: read through rd())
    if fmt == "planes":
        p = buf.view(np.int16)
        return {"hi": p[:n].reshape(shape), "lo": p[n:].reshape(shape)}
    if fmt == "mix":
        return {"hi": buf[:2 * n].view(np.int16).reshape(shape), "l": buf[2 * n:3 * n].reshape(shape), "q": buf[3 * n:].reshape(shape)}
    raise ValueError(fmt)


def rd(a, shape):
    """A plane of raw() in the image's shape, for reading (a copy: the x3 planes come as strided [..., C / 32, 32] views)."""
    return np.ascontiguousarray(a).reshape(shape)


def values(planes, fmt, layout, shape, scale=1.0, scale2=1.0):
    """Plane name -> float64 tensor of ``shape``: what the bytes hold (e4m3 bytes divided by their scale)."""
    out = {}
    for k, a in planes.items():
        a = rd(a, shape)
        if fmt == "f32":
            out[k] = torch.from_numpy(a).view(torch.float32).double()
        elif fmt == "e4m3":
            out[k] = e4m3_val(a) / scale
        elif fmt == "mix":
            out[k] = val16(a, "fp16") if k == "hi" else e4m3_val(a) / (scale if k == "l" else scale2)
        else:
            out[k] = val16(a, layout)
    return out


def encode(v, fmt, layout, scale=1.0, scale2=1.0):
    """float64 values (as the kernel's fp32 result) -> plane name -> integer ndarray, by the rules of conv1.hip / conv2.hip."""
    if fmt == "f32":
        return {"v": v.float().view(torch.int32).numpy()}
    if fmt == "16":
        return {"v": bits16(v, layout)}
    if fmt == "e4m3":
        return {"v": e4m3_bits(v.float().double() * scale)}
    if fmt in ("x3", "planes"):
        hi = r16(v, layout)
        return {"hi": bits16(hi, layout), "lo": bits16(v.float().double() - hi, layout)}
    if fmt == "mix":
        hi = r16(v, "fp16")
        return {"hi": bits16(hi, "fp16"), "l": e4m3_bits((v.float().double() - hi).float().double() * scale),
                "q": e4m3_bits(v.float().double() * scale2)}
    raise ValueError(fmt)


def put(planes, enc, where=None):
    """Write encoded planes into raw() views, at the cells of boolean mask ``where`` (the leading dimensions) or everywhere."""
    for k, a in planes.items():
        e = enc[k].reshape(a.shape)
        if where is None:
            a[...] = e
        else:
            a[where] = e[where]


def views(val, fmt, layout, scale=1.0, scale2=1.0):
    """What is compared with the float64 reference: view name -> float64 tensor."""
    if fmt in ("f32", "16", "e4m3"):
        return {"v": val["v"]}
    if fmt in ("x3", "planes"):
        return {"hi+lo": val["hi"] + val["lo"]}
    return {"hi": val["hi"], "hi+l": val["hi"] + val["l"], "q": val["q"]}


def view_bounds(ref, d, fmt, layout, scale=1.0, scale2=1.0, hi=None):
    """view name -> (reference, bound) given the fp64 result ``ref`` and the bound ``d`` of the kernel's fp32 value.  ``hi``: the
    hi plane the launch wrote (MIX: the l byte rounds what is left of the value behind it)."""
    a = ref.abs() + d
    if fmt == "f32":
        return {"v": (ref, d)}
    if fmt == "16":
        return {"v": (ref, d + 0.5 * ulp(a, layout))}
    if fmt == "e4m3":
        sat = ref.clamp(max=448.0 / scale)
        return {"v": (sat, d + 0.5 * ulp(a.clamp(max=448.0 / scale) * scale, "e4m3") / scale)}
    if fmt in ("x3", "planes"):  # |v - hi - lo| <= ulp(lo) / 2 <= u^2 |v|, one subnormal step where lo has left the normal range
        u = 2.0 ** -(MANT[layout][0] + 1)
        return {"hi+lo": (ref, d + u * u * a + 0.5 * 2.0 ** (MANT[layout][1] - MANT[layout][0]))}
    left = (ref - hi).abs() + d  # MIX: hi = half(v); l = e4m3((v - hi) S_l); q = e4m3(v S_q), saturating
    return {"hi": (ref, d + 0.5 * ulp(a, "fp16")),
            "hi+l": (ref, d + 0.5 * ulp(left * scale, "e4m3") / scale),
            "q": (ref.clamp(max=448.0 / scale2), d + 0.5 * ulp(a.clamp(max=448.0 / scale2) * scale2, "e4m3") / scale2)}


# ================================================================================================ float64 models
def conv64(img, w, drop=None):
    """3x3 / stride 2 / padding 1 without bias: img [B][Ci][H][W], w [Co][Ci][3][3] float64 -> [B][Co][H1][W1].  drop = (kh, kw,
    mask [H1][W1]): that tap's contribution is left out at the masked outputs (a mistake)."""
    out = Fn.conv2d(img, w, stride=2, padding=1)
    if drop is not None:
        kh, kw, mask = drop
        w1 = torch.zeros_like(w)
        w1[:, :, kh, kw] = w[:, :, kh, kw]
        out = out - Fn.conv2d(img, w1, stride=2, padding=1) * mask
    return out


def drop_of(bad, H, W):
    """The dropped tap of a border mistake on an [H][W] input: the one tap that reads the first / last row / column."""
    H1, W1 = sub(H), sub(W)
    m = torch.zeros(H1, W1, dtype=torch.float64)
    if "tap_dropped_top" in bad:
        m[0, :] = 1
        return (1, 1, m)
    if "tap_dropped_left" in bad:
        m[:, 0] = 1
        return (1, 1, m)
    if "tap_dropped_bottom" in bad:  # the tap that reads row H - 1: kh = 2 of the last output row when H is even, else kh = 1
        m[H1 - 1, :] = 1
        return (2 if H % 2 == 0 else 1, 1, m)
    if "tap_dropped_right" in bad:
        m[:, W1 - 1] = 1
        return (1, 2 if W % 2 == 0 else 1, m)
    return None


def expand_meta(subs, B, mistakes=()):
    """expand_meta_kernel (rowops.hip): (rows, frames) per batch -> B records (frames, tp, sub_lo, sub_hi), int32 [B][4]."""
    out = np.zeros((B, 4), np.int32)
    for b in range(B):
        lo = k = 0
        while k < len(subs) - 1 and (b > lo + subs[k][0] if "record_of_wrong_batch" in mistakes else b >= lo + subs[k][0]):
            lo += subs[k][0]
            k += 1
        T = subs[k][1]
        out[b] = (T, sub(sub(T)), lo, lo + subs[k][0])
    return out


def conv1_model(c, layout, x, frames, b0=0, mistakes=(), want_ref=True):
    """conv1 of utterances x [n][T][F] (float32; NaN where the launch must not read) with per-utterance ``frames`` [n].
    -> dict(ref, d, acc: float64 [n][T1][F1][C] or None; emu: the emulation's fp32 values as float64; own: t1_own [n])."""
    bad = set(mistakes)
    n, T, F = x.shape
    C, T1, F1 = c["C"], sub(T), sub(F)
    w9c, bias = weights1(C)
    w = w9c.double().t().reshape(C, 1, 3, 3)
    b = bias.double()
    own = np.array([sub(int(f)) for f in frames])
    X = x.double().clone()
    rows_t = torch.arange(T)[None, :, None]
    fr = torch.as_tensor(np.asarray(frames))[:, None, None]
    Xz = torch.where(rows_t < fr, X, torch.zeros_like(X))
    live = (torch.arange(T1)[None, :] < torch.as_tensor(own)[:, None])[:, :, None, None]  # [n][T1][1][1]
    out = {"own": own}
    mfma = c["form"] in ("f8m", "m16")
    s_img = c["scale"] if c["form"] == "f8m" else 1.0  # (the matrix-core e4m3 form folds the scale into w and the bias)
    if want_ref:
        pre = (conv64(Xz[:, None], w) + b[None, :, None, None]).permute(0, 2, 3, 1)
        S = (conv64(Xz[:, None].abs(), w.abs()) + b.abs()[None, :, None, None]).permute(0, 2, 3, 1)
        sq = conv64(Xz[:, None] ** 2, w ** 2).permute(0, 2, 3, 1)
        if mfma:
            u = 2.0 ** -(MANT[layout][0] + 1)
            usub = 0.5 * 2.0 ** (MANT[layout][1] - MANT[layout][0]) if layout == "fp16" else 0.0
            sw = (w.abs().sum((1, 2, 3)) + 1)[None, None, None, :]                       # sum |w| + the bias' constant one
            sx = Fn.avg_pool2d(Fn.pad(Xz[:, None].abs(), (1, 1, 1, 1)), 3, stride=2, divisor_override=1)[:, :, :T1, :F1].permute(0, 2, 3, 1)
            # hi + lo misses a value by u^2 |v| (by half a subnormal step where lo is subnormal: x against sum |w|, w s_img and the
            # bias against sum |x| + 1), the dropped lo . lo is u^2 |x||w| more
            d = 3.2 * u * u * S + usub * (sw + (sx + 1) / s_img) + 2 * gamma(30) * S
        else:
            d = gamma(10) * S
        d = torch.where(pre < -d, torch.zeros_like(d), d)  # (a ReLU whose input is negative beyond its bound gives an exact 0)
        ref = torch.relu(pre)
        acc = torch.where(ref > 0, EPS * math.sqrt(30 if mfma else 10) * (pre.abs() + sq.sqrt()), torch.zeros_like(ref))
        out.update(ref=ref * live, d=d * live, acc=acc * live)
    # ---- the emulation: the stage's roundings, float64 sums; mistakes change this only
    Xe = X if "frames_past_read" in bad else Xz
    we = w.transpose(2, 3) if "taps_transposed" in bad else w
    be = torch.zeros_like(b) if "bias_missing" in bad else b
    drop = drop_of(bad, T, F)
    if mfma:
        xh, xl = split16(Xe[:, None], layout)
        wh, wl = split16(we * s_img, layout)
        bh, bl = split16(be * s_img, layout)
        pre_e = conv64(xh, wh, drop) + conv64(xh, wl, drop) + conv64(xl, wh, drop) + (bh + bl)[None, :, None, None]
        pre_e = pre_e / s_img
    else:
        pre_e = conv64(Xe[:, None], we, drop) + be[None, :, None, None]
    pre_e = pre_e.permute(0, 2, 3, 1).float().double()
    emu = pre_e if "relu_missing" in bad else torch.relu(pre_e)
    if "t1_own_from_T" not in bad:
        emu = emu * live
    out["emu"] = emu
    return out


def rows_model(A, W, bias, K, relu, split_drop=None, emu_terms=None, mistakes=()):
    """A product of rows on the operands the kernel is GIVEN (float64 values of their bytes): out = epi(A . W^T + bias).
    A [M][K], W [N][K], split_drop = (A_lo, W_lo): the lo . lo products a split form leaves out.  emu_terms: the products the
    kernel's arithmetic sums (list of (A, W) pairs) where that is not A . W^T itself (MIX).  -> (ref, d, emu_pre, acc)."""
    bad = set(mistakes)
    p = A @ W.t()
    pre = p + bias
    S = A.abs() @ W.abs().t() + bias.abs()
    Ka = 3 * K if split_drop is not None else K  # (a split form sums three products per term)
    d = 2 * gamma(Ka + 1) * S
    if split_drop is not None:
        d = d + split_drop[0].abs() @ split_drop[1].abs().t()
    acc = EPS * math.sqrt(Ka) * (pre.abs() + ((A * A) @ (W * W).t()).sqrt())
    if emu_terms is not None:
        pe_ = sum(a @ w.t() for a, w in emu_terms)
    elif split_drop is not None:
        pe_ = p - split_drop[0] @ split_drop[1].t()
    else:
        pe_ = p
    if "e4m3_scale_off_by_one" in bad:
        pe_ = pe_ * 2
    emu = pe_ + (0.0 if "bias_missing" in bad else bias)
    if relu:
        d = torch.where(pre < -d, torch.zeros_like(d), d)
        acc = torch.where(pre > 0, acc, torch.zeros_like(acc))
        pre = torch.relu(pre)
        if "relu_missing" not in bad:
            emu = torch.relu(emu.float().double())
    return pre, d, emu.float().double(), acc


# ================================================================================================ weights and inputs
_W = {}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def weights1(C):
    """conv1: w9c [9][C] (tap-major), bias [C] - spread so that about half the pre-activations are negative."""
    if ("w1", C) not in _W:
        g = _gen(100 + C)
        _W[("w1", C)] = ((torch.randn(9, C, generator=g) / 3).contiguous(), (0.2 * torch.randn(C, generator=g)).contiguous())
    return _W[("w1", C)]


def weights2(C):
    """conv2: w [C][3][3][C] ([co][kh][kw][ci]), bias [C]."""
    if ("w2", C) not in _W:
        g = _gen(200 + C)
        _W[("w2", C)] = ((torch.randn(C, 3, 3, C, generator=g) / (3 * C ** 0.5)).contiguous(), (0.2 * torch.randn(C, generator=g)).contiguous())
    return _W[("w2", C)]


def weights_lin(K):
    if ("wl", K) not in _W:
        g = _gen(300 + K)
        _W[("wl", K)] = ((torch.randn(256, K, generator=g) / K ** 0.5).contiguous(), (0.2 * torch.randn(256, generator=g)).contiguous())
    return _W[("wl", K)]


def seed_of(c, extra=0):
    return sum(map(ord, c["name"])) * 13 + extra


def frames_of(subs, B, T):
    if subs is None:
        return np.full(B, T, np.int64)
    return expand_meta(subs, B)[:, 0].astype(np.int64)


def conv1_x(c, subs, seed):
    """x [B][T][F] float32 with NaN in every frame at or past the utterance's ``frames``."""
    B, T, F = c["B"], c["T"], c["F"]
    x = torch.randn(B, T, F, generator=_gen(seed)) * 1.5 + 0.2
    fr = frames_of(subs, B, T)
    for b in range(B):
        x[b, fr[b]:] = float("nan")
    return x, fr


# ================================================================================================ cases
FMT1 = {"planes": "planes", "mix": "mix", "f8v": "e4m3", "f8m": "e4m3", "m16": "16"}


def fmt1(c):
    return FMT1.get(c["form"], c.get("prec"))


def c1(name, site, form, B, T, F, C, halo, prec="16", subs=None, prev=None, scale=8.0, libs=None):
    """One conv1 launch.  form: plain / planes / mix / f8v / f8m / m16; prec (plain): f32 / 16 / x3; subs: the (rows, frames)
    batches of a merged pass or None; prev: the batches of an earlier halo 1 launch of the same shape into the same buffer with
    other x (halo 2 cases; () = that launch had no records)."""
    if libs is None:
        libs = LIBS if (form in ("plain", "m16") and prec == "16") else ["bf16"]
    return dict(kind="conv1", name=name, site=site, form=form, prec=prec, B=B, T=T, F=F, C=C, halo=halo, subs=subs, prev=prev, scale=scale,
                libs=[l for l in libs if l in LIBS])


def c2(name, site, form, B, T1, F1, C=256, prec="16", halo=1, out8=0.0, subs=None, c1form=None, libs=None):
    """One conv2 launch on a caller-built image of B x T1 x F1 cells - or (c1form) on the image a conv1 launch of that form writes
    into the same buffer: the hand-off.  form: generic / dma / x3 / mix / f8."""
    if libs is None:
        libs = LIBS if (form in ("generic", "dma") and prec == "16") else ["bf16"]
    return dict(kind="conv2", name=name, site=site, form=form, prec=prec, B=B, T1=T1, F1=F1, T=2 * T1 - 1, F=2 * F1 - 1, C=C, halo=halo, out8=out8, subs=subs, c1form=c1form, scale=8.0, libs=[l for l in libs if l in LIBS])


def lin(name, site, form, M, K, lda=None, pe=True, period=7, prec="16", libs=None):
    if libs is None:
        libs = LIBS if prec == "16" and form != "f8" else ["bf16"]
    return dict(kind="linear", name=name, site=site, form=form, prec=prec, M=M, K=K, lda=lda or K, pe=pe, period=period, a_scale=8.0,
                libs=[l for l in libs if l in LIBS])


RECORDS = [(1, 1), (2, 2), (1, 7), (2, 8), (1, 13)]   # frames of 1, 2, odd, even and == T (T = 13), several batches per call


def _cases():
    out = []
    # ---- conv1, VALU kernel (model.hip:112 launch_conv1; :106 planes; :103 mix planes; :108 e4m3): C changes the positions per
    # pass, T in {1, 2, odd, even}, F in {6, 7, 80, 83}
    for C, T, F in ((64, 1, 6), (64, 2, 7), (256, 9, 80), (256, 10, 83), (64, 5, 83), (256, 2, 6)):
        for prec in ("16", "f32"):
            out.append(c1(f"conv1_valu_{prec}-C{C}-T{T}-F{F}", "model.hip:112", "plain", 2, T, F, C, 0, prec))
        out.append(c1(f"conv1_valu_16_halo1-C{C}-T{T}-F{F}", "model.hip:112 (halo)", "plain", 2, T, F, C, 1))
    out.append(c1("conv1_valu_x3-C64-T9-F7", "model.hip:112 (split-bf16)", "plain", 2, 9, 7, 64, 0, "x3"))
    out.append(c1("conv1_valu_x3-C256-T10-F80", "model.hip:112 (split-bf16)", "plain", 2, 10, 80, 256, 0, "x3"))
    for form, site in (("planes", "model.hip:106"), ("mix", "model.hip:103"), ("f8v", "model.hip:108 (VALU)")):
        out.append(c1(f"conv1_{form}-C256-T9-F7", site, form, 2, 9, 7, 256, 1, scale=2.0 ** MIX_LG_AL if form == "mix" else 8.0))
        out.append(c1(f"conv1_{form}-C64-T10-F80", site, form, 2, 10, 80, 64, 1, scale=2.0 ** MIX_LG_AL if form == "mix" else 8.0))
    # grid-stride: more than 2048 image rows, every output type
    for form, prec in (("plain", "16"), ("plain", "f32"), ("plain", "x3"), ("planes", "16"), ("mix", "16"), ("f8v", "16")):
        out.append(c1(f"conv1_{form}_{prec}_gridstride-C64-T1400-F5", "conv1 row loop (> 2048 rows)", form, 3, 1400, 5, 64,
                      0 if form == "plain" else 1, prec, scale=2.0 ** MIX_LG_AL if form == "mix" else 8.0))
    # ---- merged passes: records on every conv1 form, then halo 2 after a halo 1 launch of the same shape with other x and records
    rec_forms = (("plain", "16", 64, 7), ("plain", "f32", 64, 7), ("plain", "x3", 64, 7), ("planes", "16", 256, 7), ("mix", "16", 256, 7),
                 ("f8v", "16", 256, 7), ("f8m", "16", 256, 61), ("m16", "16", 256, 61))
    for form, prec, C, F in rec_forms:
        sc = 2.0 ** MIX_LG_AL if form == "mix" else 8.0
        halo = 0 if (form == "plain" and prec != "16") else 1
        out.append(c1(f"conv1_{form}_{prec}_records-C{C}-T13-F{F}", "model.hip:101 (merged pass)", form, 7, 13, F, C, halo, prec, subs=RECORDS, scale=sc))
        if form in ("f8m", "m16") or (form == "plain" and prec == "x3"):
            continue
        prev = [(3, 13), (2, 5), (2, 9)]  # rows 3 .. 6 of the image were inside those batches; with RECORDS most are past them
        h0 = f"conv1_{form}_{prec}_halo2-C{C}-T13-F{F}"
        out.append(c1(h0, "model.hip:99 (same shape: halo mode 2)", form, 7, 13, F, C, 2, prec, subs=RECORDS, prev=prev, scale=sc))
    out.append(c1("conv1_plain_16_halo2_norecords-C64-T10-F6", "model.hip:99 (same shape: halo mode 2)", "plain", 2, 10, 6, 64, 2, prev=()))
    # ---- conv1 on the matrix cores (model.hip:108 e4m3, :110 bf16): F = 59 blocks align to rows, 61 / 62 five rows per block,
    # 80 last block partial, 126 the staging limit
    for F, T in ((59, 6), (61, 9), (62, 10), (80, 1), (80, 7), (126, 2), (126, 5)):
        out.append(c1(f"conv1_f8m-T{T}-F{F}", "model.hip:108", "f8m", 2, T, F, 256, 1))
        out.append(c1(f"conv1_m16-T{T}-F{F}", "model.hip:110", "m16", 2, T, F, 256, 1))
    # more than 1024 blocks: 36 utterances of 30 blocks ((117 + 2) rows + ... of 32 cells = 3808 cells), so workgroup g takes blocks
    # g and g + 1024 of different utterances, the deferred store crossing both boundaries; with records
    big = [(9, 233), (9, 101), (9, 2), (9, 180)]
    out.append(c1("conv1_f8m_gridstride-B36-T233-F59", "conv1_mfma_kernel block loop (> 1024 blocks)", "f8m", 36, 233, 59, 256, 1, subs=big))
    out.append(c1("conv1_m16_gridstride-B36-T233-F59", "conv1_mfma_kernel block loop (> 1024 blocks)", "m16", 36, 233, 59, 256, 1, subs=big))
    # ---- conv2 tile forms (256 output rows per tile): M < 256, M not a multiple of 256, a tile across an utterance boundary with
    # F2 = 20, both parities of T1 and F1 (the odd ones read the bottom and right halo)
    for form, site, kw in (("dma", "model.hip:149 -> gemm.hip:354", {}), ("generic", "model.hip:149 (bordered)", {}),
                           ("x3", "model.hip:144", {}), ("mix", "model.hip:141", {}), ("f8", "model.hip:147", {}),
                           ("f8", "model.hip:147 (e4m3 rows)", {"out8": 8.0})):
        tag = form + ("_out8" if kw else "")
        for B, T1, F1 in ((1, 5, 6), (3, 9, 39), (4, 10, 40)):  # M = 9; 300 (F2 = 20, tile 0 ends inside utterance 2); 400
            out.append(c2(f"conv2_{tag}-B{B}-T1{T1}-F1{F1}", site, form, B, T1, F1, **kw))
    # the real conv1 -> conv2 hand-off, halo 1 and halo 2, with records
    for c1form, form, site in (("plain", "dma", "model.hip:112 -> :149"), ("m16", "dma", "model.hip:110 -> :149"), ("planes", "x3", "model.hip:106 -> :144"),
                               ("mix", "mix", "model.hip:103 -> :141"), ("f8v", "f8", "model.hip:108 -> :147"), ("f8m", "f8", "model.hip:108 -> :147")):
        for halo in (1, 2):
            if halo == 2 and c1form in ("m16", "f8m"):
                continue
            out.append(c2(f"handoff_{c1form}_{form}_halo{halo}-B7-T13-F61", site, form, 7, 7, 31, halo=halo, subs=RECORDS, c1form=c1form))
    # ---- generic implicit GEMM: C in {64, 128} in every precision, fp32 at 256
    for prec in ("16", "f32", "x3"):
        for C in (64, 128):
            out.append(c2(f"conv2_generic_{prec}-C{C}-B2-T19-F17", "model.hip:149 (generic)", "generic", 2, 9, 7, C, prec, halo=0))
    out.append(c2("conv2_generic_f32-C256-B2-T16-F18", "model.hip:149 (generic)", "generic", 2, 6, 8, 256, "f32", halo=0))
    # ---- linear_out: K in {128, 1024, 5120}, M in {1, 257}, padded lda, pe null, pe_period not dividing M
    for K in (128, 1024, 5120):
        for M in (1, 257):
            out.append(lin(f"linear_dma-M{M}-K{K}", "model.hip:175 -> gemm.hip:358", "dma", M, K, lda=K + 64))
            out.append(lin(f"linear_generic_16-M{M}-K{K}", "model.hip:175", "generic", M, K, lda=K + 64, pe=(K != 1024)))
    out.append(lin("linear_dma_nope-M257-K1024", "model.hip:170 (conformer: no PE)", "dma", 257, 1024, pe=False))
    for prec in ("f32", "x3"):
        out.append(lin(f"linear_generic_{prec}-M257-K1024", "model.hip:175", "generic", 257, 1024, lda=1024 + 64, prec=prec))
        out.append(lin(f"linear_generic_{prec}-M1-K128", "model.hip:175", "generic", 1, 128, prec=prec))
    out.append(lin("linear_f8-M1-K5120", "model.hip:155", "f8", 1, 5120))
    out.append(lin("linear_f8-M257-K5120", "model.hip:155", "f8", 257, 5120))
    out.append(lin("linear_f8_nope-M257-K5120", "model.hip:155 (no PE)", "f8", 257, 5120, pe=False))
    return out


CASES = _cases()


class LaunchError(AssertionError):
    """A launch that fails its checks.  kind: "exact", "untouched", "bound" or "ratio"; ratio: the rms ratio of a "bound" or "ratio"
    failure."""

    def __init__(self, kind, text, ratio=None):
        super().__init__(text)
        self.kind, self.ratio = kind, ratio


def rms(t):
    return float(t.pow(2).mean().sqrt()) if t.numel() else 0.0


def compare(label, layout, got, ref, bound, emu, acc, mask, worst=None, key=None, oldnorm=None):
    """The per-element bound and the aggregate check on the elements of ``mask``."""
    g, r, b, e, a = got[mask], ref[mask], bound[mask], emu[mask], acc[mask]
    err = (g - r).abs()
    okm = err <= b
    bratio = float((err / b.clamp(min=1e-300)).nan_to_num(nan=float("inf")).max()) if g.numel() else 0.0
    yard = (rms(e - r) ** 2 + rms(a) ** 2) ** 0.5
    ratio = rms(g - r) / yard if yard > 0 else (0.0 if rms(g - r) == 0 else float("inf"))
    if oldnorm is not None and g.numel():
        oldnorm.append(float((g - r).abs().nan_to_num(nan=float("inf")).max() / r.abs().max().clamp(min=1e-300)))
    allowed = RATIO[layout]["f32" if key[2] == "f32" else "rounded"]
    if worst is not None and bool(okm.all()):
        old = worst.get(key, (0.0, 0.0))
        worst[key] = (max(old[0], bratio), max(old[1], ratio))
    if not bool(okm.all()):
        at = int((~okm).nonzero()[0])
        raise LaunchError("bound", f"{label}: |err| {float(err[at]):.3e} > bound {float(b[at]):.3e} at live element {at}; got {float(g[at]):.6g}, "
                          f"fp64 {float(r[at]):.6g}; {int((~okm).sum())} of {g.numel()} elements out of bound; rms ratio {ratio:.3g}", ratio)
    if not ratio <= allowed:
        raise LaunchError("ratio", f"{label}: rms(result - fp64) {rms(g - r):.3e} is {ratio:.3f} x the yardstick {yard:.3e} "
                          f"(emulation {rms(e - r):.3e}); allowed {allowed}", ratio)


# ================================================================================================ buffers and checks: conv1
def guarded(nbytes, fill):
    """A byte buffer of nbytes between two guards: (whole uint8 ndarray, view of the inner bytes).  The guards hold ``fill``."""
    whole = np.full(GUARD + nbytes + GUARD, fill, np.uint8)
    return whole, whole[GUARD:GUARD + nbytes]


def inner(whole):
    return whole[GUARD:whole.size - GUARD]


def img_shape(c, halo):
    h = 1 if halo else 0
    return (c["B"], sub(c["T"]) + 2 * h, sub(c["F"]) + 2 * h, c["C"])


def cell_masks(c, own, halo):
    """(live, zero, keep): boolean [B][H][W] - cells compared with the model, cells that must be bit-zero, cells that must keep
    the caller's bytes (the border under halo mode 2)."""
    B, H, W, _ = img_shape(c, halo)
    h = 1 if halo else 0
    r, q = np.arange(H)[None, :, None] - h, np.arange(W)[None, None, :] - h
    interior = np.broadcast_to((r >= 0) & (r < H - 2 * h) & (q >= 0) & (q < W - 2 * h), (B, H, W))
    live = interior & (r < np.asarray(own)[:, None, None])
    if halo == 2:
        return live, interior & ~live, ~interior
    return live, ~live, np.zeros((B, H, W), bool)


def scales_of(c):
    """(scale, scale2) of the e4m3 planes of conv1 case ``c``'s image."""
    if fmt1(c) == "mix":
        return 2.0 ** MIX_LG_AL, 2.0 ** MIX_LG_AQ
    return (c["scale"], 1.0) if fmt1(c) == "e4m3" else (1.0, 1.0)


def own_rows(frames):
    return np.array([sub(int(f)) for f in frames])


def emulate_conv1(c, layout, img, x, frames, halo, mistakes=(), chunk=8):
    """What a conv1 launch leaves in the image bytes ``img`` (the inner bytes, in place): a stand-in for the kernel on the CPU."""
    bad = set(mistakes)
    fmt, shape = fmt1(c), img_shape(c, halo)
    B, H, W, C = shape
    h = 1 if halo else 0
    s1, s2 = scales_of(c)
    planes = raw(img, fmt, shape)
    own_true = own_rows(frames)
    live, zero, _ = cell_masks(c, np.full(B, H - 2 * h) if "t1_own_from_T" in bad else own_true, halo)
    _, zero_true, _ = cell_masks(c, own_true, halo)
    write = live | zero
    if "border_rewritten_halo2" in bad and halo == 2:
        write = np.ones_like(write)
    if "past_own_unwritten_halo2" in bad and halo == 2:
        write = write & ~zero_true
    for b0 in range(0, B, chunk):
        sl = slice(b0, min(B, b0 + chunk))
        m = conv1_model(c, layout, x[sl], frames[sl], mistakes=bad, want_ref=False)
        full = torch.zeros((sl.stop - sl.start, H, W, C), dtype=torch.float64)
        full[:, h:H - h, h:W - h] = m["emu"]
        enc = encode(full, fmt, layout, s1, s2)
        if "hi_lo_swapped" in bad and "lo" in enc:
            enc["hi"], enc["lo"] = enc["lo"], enc["hi"]
        if "mix_l_q_swapped" in bad and "l" in enc:
            enc["l"], enc["q"] = enc["q"], enc["l"]
        put({k: a[sl] for k, a in planes.items()}, enc, write[sl])
    if "halo_cell_nonzero" in bad and halo == 1:
        next(iter(planes.values()))[B - 1, H - 1, W - 1].flat[-1] = 0x3c
    if "flush_at_previous_block" in bad and c["form"] in ("f8m", "m16"):
        # the last block of 128 cells of the last utterance lands one block earlier; its own place is not written
        nb = (H * W + 127) // 128
        lo = (nb - 1) * 128
        for a in planes.values():
            cells = a[B - 1].reshape(H * W, C)
            if nb > 1:
                cells[lo - 128:lo - 128 + H * W - lo] = cells[lo:]
                cells[lo:] = np.array(-1).astype(cells.dtype)


_MODEL = {}


def check_guards(label, before, after, n):
    """Nothing outside the first n inner bytes was written."""
    if not (np.array_equal(after[:GUARD], before[:GUARD]) and np.array_equal(after[GUARD + n:], before[GUARD + n:])):
        raise LaunchError("untouched", f"{label}: bytes outside the launch's own were written")


def conv1_check(c, layout, before, after, x, frames, halo, worst=None, oldnorm=None, chunk=8, tag=""):
    """Every check of the module's docstring on a conv1 launch; ``before`` / ``after``: the whole image buffers (with guards)."""
    fmt, shape = fmt1(c), img_shape(c, halo)
    B, H, W, C = shape
    h = 1 if halo else 0
    s1, s2 = scales_of(c)
    label = f"{layout} {c['name']}{tag}"
    check_guards(label, before, after, inner(after).size)
    live, zero, keep = cell_masks(c, own_rows(frames), halo)
    pa, pb = raw(inner(after), fmt, shape), raw(inner(before), fmt, shape)
    for k in pa:
        a, b_ = rd(pa[k], shape), rd(pb[k], shape)
        nz = zero[..., None] & (a != 0)
        if bool(nz.any()):
            at = tuple(int(v[0]) for v in np.nonzero(nz))
            raise LaunchError("exact", f"{label}: plane {k} (b, row, column, channel) = {at} must be bit-zero (border, or a row past the own "
                              f"batch) and holds {int(a[at]):#x}; {int(nz.sum())} such elements")
        if bool((a[keep] != b_[keep]).any()):
            raise LaunchError("untouched", f"{label}: plane {k}: {int((a[keep] != b_[keep]).sum())} border elements were rewritten under halo mode 2")
    key = (layout, c["name"].split("-")[0] + tag, fmt)
    mid = (slice(None), slice(h, H - h), slice(h, W - h))
    for b0 in range(0, B, chunk):
        sl = slice(b0, min(B, b0 + chunk))
        mk = (c["name"], layout, tag)
        if B <= chunk and mk in _MODEL:
            m = _MODEL[mk]
        else:
            m = conv1_model(c, layout, x[sl], frames[sl])
            if B <= chunk:  # (the large cases are not kept)
                _MODEL[mk] = m
        n = sl.stop - sl.start
        val = {k: v[mid] for k, v in values({k: a[sl] for k, a in pa.items()}, fmt, layout, (n, H, W, C), s1, s2).items()}
        emu_val = values(encode(m["emu"], fmt, layout, s1, s2), fmt, layout, m["emu"].shape, s1, s2)
        lv = torch.from_numpy(np.ascontiguousarray(live[sl][mid]))[..., None].expand(m["ref"].shape)
        if "lo" in val:  # hi is the rounding of hi + lo
            okh = val["lo"].abs() <= 0.5 * ulp(val["hi"], layout)
            if not bool(okh[lv].all()):
                raise LaunchError("exact", f"{label}: |lo| > ulp(hi) / 2 at {int((~okh & lv).sum())} live elements: hi is not the 16-bit "
                                  "rounding of the value")
        bounds = view_bounds(m["ref"], m["d"], fmt, layout, s1, s2, hi=val.get("hi"))
        got_v, emu_v = views(val, fmt, layout), views(emu_val, fmt, layout)
        for name, (ref, bound) in bounds.items():
            compare(f"{label} {name}", layout, got_v[name], ref, bound, emu_v[name], m["acc"], lv, worst, key + (name,), oldnorm)


# ================================================================================================ conv2 and linear: rows
def op_values(t, prec, layout):
    """fp32 tensor -> (the value the kernel's operand holds, its lo half or None) as float64, for precision f32 / 16 / x3."""
    if prec == "f32":
        return t.double(), None
    if prec == "16":
        return r16(t.double(), layout), None
    hi, lo = split16(t.double(), layout)
    return hi + lo, lo


def img_fmt2(c):
    return {"generic": c["prec"], "dma": "16", "x3": "planes", "mix": "mix", "f8": "e4m3"}[c["form"]]


def out_fmt2(c):
    if c["form"] == "f8":
        return "e4m3" if c["out8"] > 0 else "16"
    return {"generic": c["prec"], "dma": "16", "x3": "x3", "mix": "x3"}[c["form"]]


def conv1_of(c):
    """The conv1 launch of a hand-off case."""
    return dict(c, kind="conv1", form=c["c1form"], prec="16")


def conv2_values(c):
    """The unsplit values of a caller-built image: float32 [B][T1][F1][C] >= 0 with zeros, as conv1's ReLU leaves them."""
    return torch.relu(torch.randn(c["B"], c["T1"], c["F1"], c["C"], generator=_gen(seed_of(c))) * 1.5 + 0.3)


def conv2_image(c, layout):
    """The caller-built image of a conv2 case as bytes (whole buffer with NaN guards), bordered where the form reads a border."""
    v = conv2_values(c)
    h = 1 if c["halo"] else 0
    fmt = img_fmt2(c)
    shape = (c["B"], c["T1"] + 2 * h, c["F1"] + 2 * h, c["C"])
    whole, inn = guarded(int(np.prod(shape)) * IMG_BYTES[fmt], 0xff)
    full = torch.zeros(shape, dtype=torch.float64)
    full[:, h:shape[1] - h, h:shape[2] - h] = v.double()
    s1, s2 = (2.0 ** MIX_LG_AL, 2.0 ** MIX_LG_AQ) if fmt == "mix" else (c["scale"], 1.0)
    put(raw(inn, fmt, shape), encode(full, fmt, layout, s1, s2))
    return whole


def conv2_planes(c, layout, img_whole):
    """The float64 values of the image bytes a conv2 launch is given: plane -> [B][H][W][C]."""
    h = 1 if c["halo"] else 0
    fmt = img_fmt2(c)
    shape = (c["B"], c["T1"] + 2 * h, c["F1"] + 2 * h, c["C"])
    s1, s2 = (2.0 ** MIX_LG_AL, 2.0 ** MIX_LG_AQ) if fmt == "mix" else (c["scale"], 1.0)
    val = values(raw(inner(img_whole), fmt, shape), fmt, layout, shape, s1, s2)
    if fmt == "x3":
        val = {"v": val["hi"] + val["lo"], "lo": val["lo"]}
    return val


def conv2_model(c, layout, pv, mistakes=()):
    """conv2 on the operands it is given: pv = conv2_planes(...) and the host weights as the entry packs them.
    -> dict(ref, d, emu, acc: [M][C]; q8: the four scale bytes the entry must return)."""
    bad = set(mistakes)
    B, C, T2, F2 = c["B"], c["C"], sub(c["T1"]), sub(c["F1"])
    pad = 0 if c["halo"] else 1
    w2, b2 = weights2(C)
    Wm, b = w2.reshape(C, 9 * C), b2.double()
    K = 9 * C

    def im2col(v):  # [B][H][W][C] -> [M][(kh, kw, ci)]
        u = Fn.unfold(v.permute(0, 3, 1, 2), 3, padding=pad, stride=2)            # [B][C * 9][T2 * F2], channel-major
        return u.view(B, C, 9, T2 * F2).permute(0, 3, 2, 1).reshape(B * T2 * F2, K)

    form, q8 = c["form"], [0, 0, 0, 0]
    if form == "mix":  # h_a h_w + l_a q_w + q_a l_w on the bytes
        lg = e4m3_exp(float(Wm.abs().max()))
        wh = r16(Wm.double(), "fp16")
        wq = e4m3_val(e4m3_bits(Wm.double() * 2.0 ** lg)) / 2.0 ** lg
        wl = e4m3_val(e4m3_bits((Wm.double() - wh).float().double() * 2.0 ** (lg + 11))) / 2.0 ** (lg + 11)
        terms = [(im2col(pv["hi"]), wh), (im2col(pv["l"]), wq), (im2col(pv["q"]), wl)]
        pre = sum(a @ w.t() for a, w in terms) + b
        S = sum(a.abs() @ w.abs().t() for a, w in terms) + b.abs()
        d = 2 * gamma(3 * K + 1) * S
        acc = EPS * math.sqrt(3 * K) * (pre.abs() + sum((a * a) @ (w * w).t() for a, w in terms).sqrt())
        d = torch.where(pre < -d, torch.zeros_like(d), d)
        acc = torch.where(pre > 0, acc, torch.zeros_like(acc))
        emu = (pre - b if "bias_missing" in bad else pre).float().double()
        emu = emu if "relu_missing" in bad else torch.relu(emu)
        return dict(ref=torch.relu(pre), d=d, emu=emu, acc=acc, q8=[127 - lg, 127 - MIX_LG_AL, 127 - (lg + 11), 127 - MIX_LG_AQ])
    if form == "f8":
        lg = e4m3_exp(float(Wm.abs().max()))
        Wv, Wlo = e4m3_val(e4m3_bits(Wm.double() * 2.0 ** lg)) / 2.0 ** lg, None
        q8 = [127 - lg, 127 - int(round(math.log2(c["scale"]))), 0, 0]
    else:
        Wv, Wlo = op_values(Wm, {"generic": c["prec"], "dma": "16", "x3": "x3"}[form], layout)
    if Wlo is not None:
        A = im2col(pv["hi"] + pv["lo"]) if "hi" in pv else im2col(pv["v"])
        Alo = im2col(pv["lo"])
        terms = None
        if "hi_lo_swapped" in bad:  # the image's planes exchanged: a_lo w_hi + a_lo w_lo + a_hi w_hi
            terms = [(Alo, Wv), (A - Alo, Wv - Wlo)]
        ref, d, emu, acc = rows_model(A, Wv, b, K, True, (Alo, Wlo), emu_terms=terms, mistakes=bad)
    else:
        ref, d, emu, acc = rows_model(im2col(pv["v"]), Wv, b, K, True, mistakes=bad)
    return dict(ref=ref, d=d, emu=emu, acc=acc, q8=q8)


def remap_T1_for_T2(c, rows):
    """The mistake: row m split into (b, t2, f2) with T1 in T2's place."""
    B, T1, T2, F2 = c["B"], c["T1"], sub(c["T1"]), sub(c["F1"])
    M = B * T2 * F2
    m = torch.arange(M)
    b, r = m // (T1 * F2), m % (T1 * F2)
    t2, f2 = r // F2, r % F2
    ok = (b < B) & (t2 < T2)
    out = rows[((b.clamp(max=B - 1) * T2 + t2.clamp(max=T2 - 1)) * F2 + f2)].clone()
    out[~ok] = 0
    return out


def rows_buffer(nrows, ncol, fmt):
    """The output buffer of a rows launch: nrows rows, then what a last 256-row tile and one more could reach, all SENT."""
    cap = (nrows + 255) // 256 * 256 + 256
    return guarded(cap * ncol * IMG_BYTES[fmt], SENT)[0]


def rows_write(whole, rows, nrows, fmt, layout, scale, past=False):
    """Emulated rows into the output buffer; past: the rest of the last 256-row tile as well (a mistake)."""
    ncol = rows.shape[1]
    n = nrows if not past else (nrows + 255) // 256 * 256
    full = torch.ones(n, ncol, dtype=torch.float64)
    full[:nrows] = rows
    shape = (n, ncol)
    put(raw(inner(whole)[:n * ncol * IMG_BYTES[fmt]], fmt, shape), encode(full, fmt, layout, scale))


def rows_check(layout, label, before, after, fmt, m, scale, worst=None, oldnorm=None, key=None):
    """The checks of a conv2 / linear launch on its output rows: nothing past the last row written, bound and ratio on the rest."""
    nrows, ncol = m["ref"].shape
    n = nrows * ncol * IMG_BYTES[fmt]
    check_guards(label, before, after, n)
    shape = (nrows, ncol)
    val = values(raw(inner(after)[:n], fmt, shape), fmt, layout, shape, scale)
    emu_val = values(encode(m["emu"], fmt, layout, scale), fmt, layout, shape, scale)
    lv = torch.ones(shape, dtype=torch.bool)
    if "lo" in val:
        okh = val["lo"].abs() <= 0.5 * ulp(val["hi"], layout)
        if not bool(okh.all()):
            raise LaunchError("exact", f"{label}: |lo| > ulp(hi) / 2 at {int((~okh).sum())} elements: hi is not the 16-bit rounding of the value")
    bounds = view_bounds(m["ref"], m["d"], fmt, layout, scale)
    got_v, emu_v = views(val, fmt, layout), views(emu_val, fmt, layout)
    for name, (ref, bound) in bounds.items():
        compare(f"{label} {name}", layout, got_v[name], ref, bound, emu_v[name], m["acc"], lv, worst, key + (name,), oldnorm)


LIN_SCALE = 16.0  # sqrt(d_model)


def lin_fmt(c):
    return "e4m3" if c["form"] == "f8" else c["prec"]


def linear_inputs(c, layout):
    """(the operand's float64 values [M][K], lo halves or None, the A buffer [M + 7][lda] as bytes with guards: NaN in spare columns,
    in the rows past M and around)."""
    M, K, lda = c["M"], c["K"], c["lda"]
    a = torch.randn(M, K, generator=_gen(seed_of(c))) * 1.2
    cap, fmt = M + 7, lin_fmt(c)
    whole, inn = guarded(cap * lda * IMG_BYTES[fmt], 0xff)
    pad = torch.full((cap, lda), float("nan"), dtype=torch.float64)
    if fmt == "e4m3":
        a = torch.relu(a)
        rows = inn.reshape(cap, lda)
        rows[:M, :K] = e4m3_bits(a.double() * c["a_scale"])
        return e4m3_val(rows[:M, :K]) / c["a_scale"], None, whole
    pad[:M, :K] = a.double()
    put(raw(inn, fmt, (cap, lda)), encode(pad, fmt, layout))
    val, lo = op_values(a, fmt, layout)
    return val, lo, whole


def linear_a_ignoring_lda(c, layout, a_whole):
    """The mistake: row m of A read at m K instead of m lda."""
    M, K, lda = c["M"], c["K"], c["lda"]
    fmt, shape = lin_fmt(c), (M + 7, lda)
    v = views(values(raw(inner(a_whole), fmt, shape), fmt, layout, shape, c["a_scale"]), fmt, layout)
    return next(iter(v.values())).reshape(-1)[:M * K].reshape(M, K)


def pe_table(c):
    return (torch.randn(c["period"], 256, generator=_gen(seed_of(c, 5))) * 2).contiguous() if c["pe"] else None


def linear_model(c, layout, A=None, mistakes=()):
    """linear_out on the operands it is given -> dict(ref, d, emu, acc: [M][256]; q8)."""
    bad = set(mistakes)
    M, K = c["M"], c["K"]
    w, b = weights_lin(K)
    Av, Alo, _ = linear_inputs(c, layout)
    q8 = [0, 0, 0, 0]
    if c["form"] == "f8":
        lg = e4m3_exp(float(w.abs().max()))
        Wv, Wlo = e4m3_val(e4m3_bits(w.double() * 2.0 ** lg)) / 2.0 ** lg, None
        q8 = [127 - lg, 127 - int(round(math.log2(c["a_scale"]))), 0, 0]
    else:
        Wv, Wlo = op_values(w, c["prec"], layout)
    pre, d, _, acc = rows_model(Av, Wv, b.double(), K, False, (Alo, Wlo) if Alo is not None else None)
    emu = rows_model(Av if A is None else A, Wv, b.double(), K, False, (Alo, Wlo) if (Alo is not None and A is None) else None, mistakes=bad)[2]
    pe = pe_table(c)
    rows_pe = rows_bad = torch.zeros(M, 256, dtype=torch.float64)
    if pe is not None:
        m_ = torch.arange(M)
        rows_pe = pe.double()[m_ % c["period"]]
        rows_bad = pe.double()[(m_ // c["period"]).clamp(max=c["period"] - 1)]
    ref = pre * LIN_SCALE + rows_pe
    d = d * LIN_SCALE + 2 * EPS * (pre.abs() + d) * LIN_SCALE + EPS * ref.abs()  # (sum + bias) * scale, + pe: three fp32 roundings
    emu = ((emu * LIN_SCALE).float().double() + (rows_bad if "pe_row_div" in bad else rows_pe)).float().double()
    return dict(ref=ref, d=d, emu=emu, acc=acc * LIN_SCALE, q8=q8)


# ================================================================================================ a case, launch by launch
def call_of(c, layout, stages, **kw):
    """One descriptor call: the host side of cn_op_frontend_desc.  stages: subset of conv1 / conv2 / linear; x: float32 tensor
    (conv1); img / out / a: whole byte buffers with guards; subs: the (rows, frames) list or None; pe: float32 tensor or None."""
    return dict(c=c, layout=layout, stages=stages, halo=kw.pop("halo", 0), subs=kw.pop("subs", None), **kw)


def emulate(call, mistakes=()):
    """The launcher of the CPU tests: what cn_op_frontend_desc would leave, from the emulation, with ``mistakes``."""
    bad = set(mistakes)
    c, layout, st = call["c"], call["layout"], call["stages"]
    res = {"meta": None, "q8": [0] * 8}
    if "conv1" in st:
        cc = c if c["kind"] == "conv1" else conv1_of(c)
        img = call["img"].copy()
        frames = np.full(c["B"], c["T"], np.int64)
        if call["subs"]:
            res["meta"] = expand_meta(call["subs"], c["B"], bad)
            frames = res["meta"][:, 0].astype(np.int64)
        emulate_conv1(cc, layout, inner(img), call["x"], frames, call["halo"], bad)
        res["img"] = img
    if "conv2" in st:
        img = res.get("img", call["img"])
        m = conv2_model(c, layout, conv2_planes(c, layout, img), bad)
        rows = remap_T1_for_T2(c, m["emu"]) if "row_split_T1_for_T2" in bad else m["emu"]
        out = call["out"].copy()
        rows_write(out, rows, rows.shape[0], out_fmt2(c), layout, c["out8"] or 1.0, "rows_past_M_stored" in bad)
        res.update(out=out, img=img)
        res["q8"][:4] = m["q8"]
    if "linear" in st:
        A = linear_a_ignoring_lda(c, layout, call["a"]) if "lda_ignored" in bad else None
        m = linear_model(c, layout, A, bad)
        out = call["out"].copy()
        rows_write(out, m["emu"], c["M"], "f32", layout, 1.0, "rows_past_M_stored" in bad)
        res["out"] = out
        res["q8"][4:] = m["q8"]
    return res


def border_sentinel(c, img_whole, halo=1):
    """SENT bytes into every border cell of a bordered image: what a halo mode 2 launch must leave alone."""
    shape = img_shape(c, halo)
    _, _, border = cell_masks(c, np.zeros(c["B"], int), 2)
    for a in raw(inner(img_whole), fmt1(c), shape).values():
        a[border] = np.array(0x5A5A5A5A).astype(a.dtype) if a.dtype != np.uint8 else SENT


def run_case(c, layout, launch, worst=None, oldnorm=None):
    """Case ``c`` through ``launch`` (a function of a call_of() dict that returns dict(img, out, meta, q8)) with every check."""
    label = f"{layout} {c['name']}"
    if c["kind"] == "conv1":
        n = int(np.prod(img_shape(c, c["halo"]))) * IMG_BYTES[fmt1(c)]
        img = guarded(n, SENT)[0]
        inner(img)[:] = 0xff  # NaN in every format: every cell must be written
        if c["halo"] == 2:
            xp, frp = conv1_x(c, c["prev"] or None, seed_of(c, 1))
            r = launch(call_of(c, layout, {"conv1"}, halo=1, subs=c["prev"] or None, x=xp, img=img))
            conv1_check(c, layout, img, r["img"], xp, frp, 1, tag=" (the halo 1 launch before)")
            img = r["img"].copy()
            border_sentinel(c, img)
        x, fr = conv1_x(c, c["subs"], seed_of(c))
        r = launch(call_of(c, layout, {"conv1"}, halo=c["halo"], subs=c["subs"], x=x, img=img))
        if c["subs"] and not np.array_equal(r["meta"], expand_meta(c["subs"], c["B"])):
            raise LaunchError("exact", f"{label}: expand_meta's records differ from the model's")
        conv1_check(c, layout, img, r["img"], x, fr, c["halo"], worst, oldnorm)
        return
    if c["kind"] == "conv2":
        M, fmt = c["B"] * sub(c["T1"]) * sub(c["F1"]), out_fmt2(c)
        out = rows_buffer(M, c["C"], fmt)
        if c["c1form"]:
            cc = conv1_of(c)
            n = int(np.prod(img_shape(cc, 1))) * IMG_BYTES[fmt1(cc)]
            img = guarded(n, SENT)[0]
            inner(img)[:] = 0xff
            if c["halo"] == 2:  # a halo 1 pass of the same shape with other x and records first; its border zeros stay (conv2 reads them)
                prev = [(3, 13), (2, 5), (2, 9)]
                xp, frp = conv1_x(cc, prev, seed_of(c, 1))
                r = launch(call_of(c, layout, {"conv1", "conv2"}, halo=1, subs=prev, x=xp, img=img, out=out))
                conv1_check(cc, layout, img, r["img"], xp, frp, 1, tag=" (the halo 1 pass before)")
                img = r["img"].copy()
            x, fr = conv1_x(cc, c["subs"], seed_of(c))
            r = launch(call_of(c, layout, {"conv1", "conv2"}, halo=c["halo"], subs=c["subs"], x=x, img=img, out=out))
            if not np.array_equal(r["meta"], expand_meta(c["subs"], c["B"])):
                raise LaunchError("exact", f"{label}: expand_meta's records differ from the model's")
            conv1_check(cc, layout, img, r["img"], x, fr, c["halo"], worst, oldnorm, tag=" conv1")
            m = conv2_model(c, layout, conv2_planes(c, layout, r["img"]))  # the operands are the bytes conv1 wrote
        else:
            img = conv2_image(c, layout)
            r = launch(call_of(c, layout, {"conv2"}, halo=c["halo"], img=img, out=out))
            if not np.array_equal(r["img"], img):
                raise LaunchError("untouched", f"{label}: conv2 wrote its input image")
            if (c["name"], layout) not in _MODEL:
                _MODEL[(c["name"], layout)] = conv2_model(c, layout, conv2_planes(c, layout, img))
            m = _MODEL[(c["name"], layout)]
        if list(r["q8"][:4]) != m["q8"]:
            raise LaunchError("exact", f"{label}: scale bytes {list(r['q8'][:4])}, the model's packers give {m['q8']}")
        rows_check(layout, label, out, r["out"], fmt, m, c["out8"] or 1.0, worst, oldnorm, (layout, c["name"].split("-")[0], fmt))
        return
    _, _, a = linear_inputs(c, layout)
    out = rows_buffer(c["M"], 256, "f32")
    r = launch(call_of(c, layout, {"linear"}, a=a, out=out, pe=pe_table(c)))
    if (c["name"], layout) not in _MODEL:
        _MODEL[(c["name"], layout)] = linear_model(c, layout)
    m = _MODEL[(c["name"], layout)]
    if list(r["q8"][4:]) != m["q8"]:
        raise LaunchError("exact", f"{label}: scale bytes {list(r['q8'][4:])}, the model's packers give {m['q8']}")
    rows_check(layout, label, out, r["out"], "f32", m, 1.0, worst, oldnorm, (layout, c["name"].split("-")[0], "f32"))
