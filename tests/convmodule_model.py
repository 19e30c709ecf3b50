"""float64 models of the conformer convolution module's kernels (csrc/conformer.hip: GLU, depthwise convolution over time, GroupNorm(1, C)
+ Swish) with per-element error bounds, and the seeded cases of their tests.  Shared by the kernel test (test_gpu_convmodule.py) and the
CPU test that shows the bounds hold for the arithmetic as written and are tight enough to catch the mistakes such kernels could make
(test_convmodule_model.py).

Each model takes the float64 operands as the kernel sees them in a layout (attention_model.to_layout) and returns (out, bound).  The
bounds follow the kernels' float32 arithmetic, operation by operation:

  fast exponential   relative error (2 |arg| + 4) EPS (the figure of attention_model, which the device has met); sigmoid and Swish take at
                     most that, plus the roundings of the add, the divide and the multiply
  dwconv             bias then k fused multiply-adds in tap order: gamma(k + 1) (|bias| + sum |w x|)
  GroupNorm value    v = (x - fl32(mean)) inv gw + gb: |gw| inv (|mean| EPS + 3 EPS |x - mean|) + 2 EPS |v|; the first term is the float32
                     rounding of the mean - a property of the kernel.  inv itself carries the statistics' roundoff (d_inv below).  Swish has
                     slope <= 1.1
  statistics         double sums of n values in any order: gamma64(n) sum |x| (and of x^2; a float32 squared is exact in double)
  output             the layout's rounding (out_ulp: half an ulp for bf16 / fp16, the 2^-16 relative term for split-bf16), 1e-37 for flushed
                     subnormals
  slack              the arithmetic terms times 2, as attention_model does

Condition of the GroupNorm bound: |mean| / std <= 64 (or a constant image), so that the cancellation in E[x^2] - mean^2, evaluated in
double, stays some 2^12 double roundoffs of the variance - the term d_inv accounts for it and is negligible beside EPS."""
import functools
import math

import torch

from attention_model import EPS, gamma, out_ulp, to_layout

EPS64 = 2.0 ** -53
FLOOR = 1e-37  # flushed subnormals
SLACK = 2.0
GN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))  # F.group_norm's default as the float the launcher takes

MISTAKES = ("glu_halves_swapped", "glu_gate_first_half", "dw_taps_flipped", "dw_pad_plus_one", "dw_pad_minus_one", "dw_no_bias",
            "dw_weight_transposed", "dw_leaks_across_utterances", "dw_last_tile_short", "gn_unbiased_variance", "gn_batch_statistics",
            "gn_affine_by_frame", "gn_eps_outside_sqrt", "gn_no_swish")


def gamma64(n):
    return n * EPS64 / (1 - n * EPS64)


def _bad(mistakes):
    bad = set(mistakes)
    assert bad <= set(MISTAKES), bad
    return bad


def _rounded(out, arith, layout):
    """Bound of the stored element: the arithmetic bound, the layout's output rounding at the largest magnitude inside it, the floor."""
    bound = SLACK * arith
    return bound + out_ulp(out.abs() + bound, layout) * (1.0 if layout == "bf16x3" else 0.5) + FLOOR


def _sigmoid_rel(arg):
    """Relative error of 1 / (1 + __expf(-arg)): the exponential's, the add and the divide."""
    return (2 * arg.abs() + 4) * EPS + 2 * EPS


def glu_model(x, layout, mistakes=()):
    """x (M, 2 d) -> a * sigmoid(g) with a = x[:, :d], g = x[:, d:] (F.glu over the channels): (out, bound), (M, d)."""
    bad = _bad(mistakes)
    d = x.shape[1] // 2
    a, g = x[:, :d], x[:, d:]
    if "glu_halves_swapped" in bad:
        a, g = g, a
    if "glu_gate_first_half" in bad:
        g = a
    out = a * torch.sigmoid(g)
    return out, _rounded(out, (_sigmoid_rel(g) + EPS) * out.abs(), layout)


def dwconv_model(x, w, bias, B, L, k, mistakes=(), dx=None):
    """x (B L, d), w (d, k), bias (d,) -> bias[c] + sum_j w[c][j] x[b][t + j - (k - 1) // 2][c], zero outside [0, L) of the same utterance:
    (out, bound), (B L, d) - float32 outputs in every layout.  dx: a bound on the error of x itself (a composed run), carried through."""
    bad = _bad(mistakes)
    d = x.shape[1]
    pad = (k - 1) // 2 + ("dw_pad_plus_one" in bad) - ("dw_pad_minus_one" in bad)
    if "dw_taps_flipped" in bad:
        w = w.flip(1)
    if "dw_weight_transposed" in bad:
        w = w.reshape(k, d).t()
    if "dw_no_bias" in bad:
        bias = torch.zeros_like(bias)
    if "dw_leaks_across_utterances" in bad:
        B, L = 1, B * L
    t = torch.arange(L)
    src = t[:, None] + torch.arange(k)[None, :] - pad  # (L, k): the frame tap j of output t reads
    ok = (src >= 0) & (src < L)
    if "dw_last_tile_short" in bad:
        t0 = 32 * (L // 32)
        ok &= (t[:, None] < t0) | (src >= t0)
    taps = w.t()[None, None] * ok[None, :, :, None]  # (1, L, k, d)
    idx = src.clamp(0, L - 1)

    def conv(v, wt):
        return (v.reshape(B, L, d)[:, idx] * wt).sum(2).reshape(B * L, d)

    out = conv(x, taps) + bias
    mass = conv(x.abs() + (0 if dx is None else dx), taps.abs())
    bound = SLACK * gamma(k + 1) * (bias.abs() + mass) + FLOOR
    if dx is not None:
        bound = bound + conv(dx, taps.abs())
    return out, bound


def exact_stats(x, B):
    """(B, 2) float64: each utterance's sum and sum of squares, correctly rounded (the values are float32 numbers: their squares are exact)."""
    rows = x.reshape(B, -1)
    return torch.tensor([[math.fsum(r.tolist()), math.fsum((r * r).tolist())] for r in rows], dtype=torch.float64)


def groupnorm_swish_model(x, gw, gb, B, L, eps, layout, mistakes=(), dx=None, stats=None):
    """x (B L, d) float64 of float32 values, gw / gb (d,) -> swish(gw (x - mean_b) / sqrt(var_b + eps) + gb), mean and biased variance over
    the whole L x d image of utterance b (F.group_norm(x, 1)): (out, bound, stats, stats_bound); stats (B, 2) = (sum, sum of squares) and
    their bound.  dx: a bound on the error of x itself (a composed run), carried through mean, variance and value.  stats: exact_stats(x, B)
    when the caller has it already."""
    bad = _bad(mistakes)
    d = x.shape[1]
    n = L * d
    img = x.reshape(B, n)
    stats = exact_stats(x, B) if stats is None else stats
    stats_bound = SLACK * gamma64(n) * torch.stack([img.abs().sum(1), (img * img).sum(1)], 1) + 1e-300
    mean = (stats[:, 0] / n)[:, None]
    var = ((img - mean) ** 2).mean(1, keepdim=True)  # (no cancellation: the model's own variance)
    if "gn_batch_statistics" in bad:
        mean = img.mean().expand(B, 1)
        var = ((img - mean) ** 2).mean().expand(B, 1)
    if "gn_unbiased_variance" in bad:
        var = var * n / max(n - 1, 1)
    inv = 1.0 / (var.sqrt() + eps) if "gn_eps_outside_sqrt" in bad else 1.0 / (var + eps).sqrt()
    # what the sums' roundoff does to inv = (S2 / n - mean^2 + eps)^(-1/2): d_var = (dS2 + 2 |mean| dS1) / n and the double roundings of
    # the two quotients, the square and the difference, each relative to mean^2 + var
    d_var = (stats_bound[:, 1:2] + 2 * mean.abs() * stats_bound[:, 0:1]) / n + 6 * EPS64 * (mean * mean + var)
    d_inv = 0.5 * d_var / (var + eps)  # relative
    cen = (img - mean).reshape(B, L, d)
    if "gn_affine_by_frame" in bad:
        tt = torch.arange(L) % d
        ga, be = gw[tt][None, :, None], gb[tt][None, :, None]
    else:
        ga, be = gw[None, None, :], gb[None, None, :]
    iv = inv[:, :, None]
    scaled = ga * cen * iv
    v = scaled + be
    dv = ga.abs() * iv * (mean.abs()[:, :, None] * EPS + 3 * EPS * cen.abs()) + 2 * EPS * v.abs() + d_inv[:, :, None] * scaled.abs()
    carried = 0
    if dx is not None:  # |d mean| <= mean(dx); sqrt(var + eps) moves by at most rms(dx - d mean) <= rms(dx) + mean(dx)
        e = dx.reshape(B, n)
        m1 = e.mean(1, keepdim=True)
        s1 = (e * e).mean(1, keepdim=True).sqrt() + m1
        sd = (var + eps).sqrt()
        assert (s1 < 0.5 * sd).all(), "the carried error is not small beside the standard deviation"
        carried = ga.abs() * ((e.reshape(B, L, d) + m1[:, :, None]) * iv + cen.abs() * (s1 / (sd * (sd - s1)))[:, :, None])
    out = v if "gn_no_swish" in bad else v * torch.sigmoid(v)
    arith = 1.1 * dv + (_sigmoid_rel(v) + EPS) * out.abs()
    bound = _rounded(out, arith + 1.1 * carried / SLACK, layout)
    return out.reshape(B * L, d), bound.reshape(B * L, d), stats, stats_bound


def conv_module_model(x, w, bias, gw, gb, B, L, k, eps, layout):
    """GLU -> dwconv -> GroupNorm + Swish as run_conv_module chains them (the GLU output is stored in the layout, the convolution's in
    float32), every stage's bound carried into the next: (out, bound).  The device convolves the GLU values it stored, which differ from
    the float64 ones by at most the GLU bound, and normalises the convolution it computed, which differs by at most the carried bound.
    (Each stage's own bound is evaluated at the float64 values; what the carried error adds to it is of second order.)"""
    g, bg = glu_model(x, layout)
    y, by = dwconv_model(g, w, bias, B, L, k, dx=bg)
    out, bound, _, _ = groupnorm_swish_model(y, gw, gb, B, L, eps, layout, dx=by)
    return out, bound


# ============================================================================================ float32 emulations (host only)
def glu_emulation(x):
    """The kernel's float32 arithmetic on float64 operands x (M, 2 d), torch.exp for the fast exponential; unrounded float32 output."""
    d = x.shape[1] // 2
    a, g = x[:, :d].float(), x[:, d:].float()
    return a * (1.0 / (1.0 + torch.exp(-g)))


def dwconv_emulation(x, w, bias, B, L, k):
    """bias, then one fused multiply-add per tap in tap order (an exact product, one rounding of the sum)."""
    d = x.shape[1]
    xb = x.reshape(B, L, d)
    pad = (k - 1) // 2
    acc = bias.float()[None, None].expand(B, L, d).clone()
    for j in range(k):
        lo, hi = max(0, pad - j), min(L, L + pad - j)  # outputs t whose frame t + j - pad exists
        if lo < hi:
            acc[:, lo:hi] = (w[:, j][None, None] * xb[:, lo + j - pad:hi + j - pad] + acc[:, lo:hi].double()).float()
    return acc.reshape(B * L, d)


def groupnorm_swish_emulation(x, gw, gb, B, L, eps):
    """Double sums, mean and E[x^2] - mean^2 in double, the mean and 1 / sqrt rounded to float32, the rest float32."""
    d = x.shape[1]
    n = L * d
    img = x.reshape(B, n)
    mean = img.sum(1) / n
    var = (img * img).sum(1) / n - mean * mean
    inv = (1.0 / (var.clamp(min=0.0) + float(torch.tensor(eps, dtype=torch.float32))).sqrt()).float()
    v = (img.float() - mean.float()[:, None]) * inv[:, None]
    v = v.reshape(B, L, d) * gw.float() + gb.float()
    return (v * (1.0 / (1.0 + torch.exp(-v)))).reshape(B * L, d)


# ============================================================================================ seeded cases (host tensors only)
GLU_SHAPES = [(1, 32), (37, 144), (300, 256), (5, 512)]  # (M, d); d = 144 has no split-bf16 layout


def splits(d):
    return d % 32 == 0


def glu_case(M, d, seed=0):
    """float32 (M, 2 d): values N(0, 1), gates N(0, 4^2) with +-30 (saturation) and +-100 (the exponential overflows / vanishes) planted in
    the first and the last row, and exact zeros in value, gate and both."""
    g = torch.Generator().manual_seed(1000 * d + M + seed)
    x = torch.randn(M, 2 * d, generator=g)
    x[:, d:] *= 4.0
    for row, c0 in ((0, 0), (M - 1, d - 8)):
        x[row, d + c0:d + c0 + 4] = torch.tensor([30.0, -30.0, 100.0, -100.0])
        x[row, c0 + 4] = 0.0
        x[row, d + c0 + 5] = 0.0
        x[row, c0 + 6] = 0.0
        x[row, d + c0 + 6] = 0.0
    return x


DW_TILED_K = (3, 7, 15, 31)  # the tiled kernel's sizes (form 0), the naive kernel's with form 1
DW_NAIVE_K = (1, 5, 9, 17)  # form 0 sends these to the naive kernel
DW_L = (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 97)
DW_D = (32, 144, 256, 288)
DW_B = 3
DW_SCALES = (1.0, 100.0, 0.01)  # per utterance: a tap that crosses a border moves the quiet neighbour far beyond its bound


def dw_shapes(k):
    """(L, d) pairs of kernel size k: every L of DW_L - and the halo (k - 1) / 2 itself with its two neighbours where DW_L lacks them - at
    d = 288 (a second, partly filled block of channels); the other widths at L = 1, 33 and 97 (one frame, a second tile of one frame, a
    fourth tile of one frame)."""
    pad = (k - 1) // 2
    Ls = sorted(set(DW_L) | {v for v in (pad - 1, pad, pad + 1) if v >= 1})
    return [(L, 288) for L in Ls] + [(L, d) for d in DW_D[:3] for L in (1, 33, 97)]


def dw_case(k, L, d, B=DW_B):
    """float32 x (B L, d) with utterance b scaled by DW_SCALES[b], w (d, k), bias (d,)."""
    g = torch.Generator().manual_seed(100000 * k + 1000 * L + d)
    x = torch.randn(B, L, d, generator=g) * torch.tensor(DW_SCALES[:B])[:, None, None]
    w = torch.randn(d, k, generator=g) * 0.5
    bias = torch.randn(d, generator=g)
    return x.reshape(B * L, d), w, bias


# (B, L, d) and the kind of each utterance: n = 32 (most of the workgroup idle), 432, 1024 exactly, 1280, 64 000, 512 000
GN_SHAPES = [((1, 1, 32), ("plain",)), ((3, 3, 144), ("offset", "const", "tiny")), ((2, 4, 256), ("plain", "offset")),
             ((3, 5, 256), ("tiny", "offset", "const")), ((2, 250, 256), ("offset", "plain")), ((2, 1000, 512), ("const", "offset"))]
GN_KINDS = {"plain": (0.3, 2.0), "offset": (32.0, 0.5), "tiny": (0.02, 1e-3), "const": (-1.75, 0.0)}  # mean, std: |mean| / std <= 64


def gn_case(B, L, d, kinds):
    """float32 x (B L, d): utterance b is N(mean, std^2) of its kind ("offset": the float32 rounding of the mean is the visible part of the
    bound; "const": zero variance; "tiny": a variance below eps), gamma around 1, beta around 0."""
    g = torch.Generator().manual_seed(1000 * L + d + B)
    x = torch.randn(B, L, d, generator=g)
    for b, kind in enumerate(kinds):
        mean, std = GN_KINDS[kind]
        x[b] = x[b] * std + mean
    gw = 1.0 + 0.3 * torch.randn(d, generator=g)
    gb = 0.5 * torch.randn(d, generator=g)
    return x.reshape(B * L, d), gw, gb


SEQ_SHAPE = dict(B=2, L=65, d=256, k=15)


def seq_case():
    """The three kernels in sequence: float32 x (B L, 2 d) in front of the GLU, w, bias, gamma, beta."""
    B, L, d, k = (SEQ_SHAPE[n] for n in ("B", "L", "d", "k"))
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B * L, 2 * d, generator=g)
    x[:, d:] *= 2.0
    x[L:] *= 3.0  # (the second utterance: its own statistics)
    w = torch.randn(d, k, generator=g) * 0.4
    bias = torch.randn(d, generator=g) * 0.5
    gw = 1.0 + 0.3 * torch.randn(d, generator=g)
    gb = 0.5 * torch.randn(d, generator=g)
    return x, w, bias, gw, gb


# ============================================================================================ references, computed once per session
@functools.lru_cache(maxsize=None)
def dw_reference(layout, k, L, d):
    """(x32, w32, bias32, float64 operand x, w, bias, out, bound) of dw_case(k, L, d) in ``layout``; shared, not to be modified."""
    x32, w32, b32 = dw_case(k, L, d)
    x = to_layout(x32, layout, device="cpu")[1]
    return (x32, w32, b32, x, w32.double(), b32.double()) + dwconv_model(x, w32.double(), b32.double(), DW_B, L, k)


@functools.lru_cache(maxsize=None)
def gn_reference(i):
    """(x32, gw32, gb32, float64 x, gw, gb, exact stats) of GN_SHAPES[i]; shared, not to be modified."""
    (B, L, d), kinds = GN_SHAPES[i]
    x32, gw32, gb32 = gn_case(B, L, d, kinds)
    return x32, gw32, gb32, x32.double(), gw32.double(), gb32.double(), exact_stats(x32.double(), B)
