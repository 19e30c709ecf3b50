"""The conformer convolution module's kernels (csrc/conformer.hip: glu_kernel, dwconv_kernel, dwconv_tiled_kernel, groupnorm_stats_kernel,
groupnorm_swish_kernel), each driven alone through cn_op_glu / cn_op_dwconv / cn_op_groupnorm_swish and compared with the float64 models
of convmodule_model.py within their per-element bounds, and bit for bit against themselves: the tiled depthwise convolution against the
naive one, and every utterance of a batch against the same utterance run alone.

Every input sits inside a larger NaN-filled allocation (guard rows before and after - k of them around the convolution's frames - and
spare floats around the weight vectors), every output inside a sentinel-filled one whose guard region must come back untouched.  The
shapes are the smallest at which each thing can go wrong (convmodule_model.py holds them; test_convmodule_model.py shows on the host that
the bounds at these shapes would catch each mistake of MISTAKES).

Run with -s to see the worst error / bound ratio per kernel, layout and form.

Worst |out - fp64| / bound recorded on an MI355X (74 tests, under 4 s); where the stored element is bf16 / fp16 its own rounding - half an
ulp - is nearly the whole bound, so a ratio just below 1 is the expected figure there:

  kernel     layout   form    ratio   |err|          kernel     layout   form    ratio   |err|
  dwconv     fp32     tiled   0.345   3.49e-05       glu        fp32     -       0.249   3.28e-07
  dwconv     fp32     naive   0.345   3.49e-05       glu        bf16     -       1.000   7.81e-03
  dwconv     bf16     tiled   0.354   3.46e-05       glu        fp16     -       0.999   9.76e-04
  dwconv     bf16     naive   0.365   4.95e-05       glu        bf16x3   -       0.462   1.54e-05
  dwconv     fp16     tiled   0.347   3.69e-05       gn_swish   fp32     -       0.281   4.58e-06
  dwconv     fp16     naive   0.347   3.69e-05       gn_swish   bf16     -       0.999   1.55e-02
  dwconv     bf16x3   tiled   0.348   2.84e-05       gn_swish   fp16     -       0.996   1.93e-03
  dwconv     bf16x3   naive   0.348   2.84e-05       gn_swish   bf16x3   -       0.450   3.08e-05
  gn_stats   -        -       0.028   2.84e-14       sequence   fp32 0.022, bf16 0.456, fp16 0.460, bf16x3 0.154

The tiled depthwise convolution equalled the naive one bit for bit at every shape, as the comment in conformer.hip claims."""
import pytest
import torch

import convmodule_model as cm
from attention_model import LAYOUTS, from_layout, to_layout
from cassnat_asr_public_amd import hip

pytestmark = pytest.mark.gpu

LAYOUT_NAMES = list(LAYOUTS)
SENTINEL = 7.0
NAN = float("nan")
SPARE = 16  # floats around a weight vector
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    print("\nworst |out - fp64| / bound per kernel, layout and form:")
    for (kernel, layout, form), (ratio, err) in sorted(WORST.items()):
        print(f"  {kernel:10s} {layout:7s} {form:6s} {ratio:.3f}  (|err| {err:.2e})")


def lib_of(layout):
    flavour, prec, operand = LAYOUTS[layout]
    L = hip.lib(flavour)
    assert L.cn_operand16().decode() == operand
    return L, prec


def layouts_for(d):
    return [n for n in LAYOUT_NAMES if n != "bf16x3" or cm.splits(d)]


def bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Rows:
    """R rows of ``cols`` elements in a layout on the device, with ``guard`` rows of ``fill`` before and after."""

    def __init__(self, x32, layout, guard, fill=NAN, rows=None, cols=None):
        R, Cn = (rows, cols) if x32 is None else x32.shape
        full = torch.full((R + 2 * guard, Cn), fill)
        if x32 is not None:
            full[guard:guard + R] = x32
        self.layout, self.guard, self.R = layout, guard, R
        self.dev = to_layout(full, layout)[0]
        self.before = self.dev.clone()
        self.ptr = self.dev.data_ptr() + guard * self.dev.shape[1] * self.dev.element_size()

    def body(self):
        return self.dev[self.guard:self.guard + self.R]

    def value(self):
        """(float64 values, raw bits) of the rows, after checking that the guard rows are what they were."""
        g = self.guard
        assert torch.equal(bits(self.dev[:g]), bits(self.before[:g])), "a row in front of the output was written"
        assert torch.equal(bits(self.dev[g + self.R:]), bits(self.before[g + self.R:])), "a row behind the output was written"
        return from_layout(self.body(), self.layout), bits(self.body().cpu())


class Vec:
    """A float32 / float64 vector on the device with SPARE elements of ``fill`` on either side."""

    def __init__(self, v, fill=NAN):
        full = torch.full((v.numel() + 2 * SPARE,), fill, dtype=v.dtype)
        full[SPARE:SPARE + v.numel()] = v.reshape(-1)
        self.n = v.numel()
        self.dev = full.cuda()
        self.before = self.dev.clone()
        self.ptr = self.dev.data_ptr() + SPARE * self.dev.element_size()

    def value(self):
        assert torch.equal(bits(self.dev[:SPARE]), bits(self.before[:SPARE])) and torch.equal(bits(self.dev[SPARE + self.n:]), bits(self.before[SPARE + self.n:])), \
            "an element beside the output was written"
        return self.dev[SPARE:SPARE + self.n].cpu()


def run_glu(layout, x32, out=None):
    """x32 (M, 2 d) -> Rows of the output (M, d)."""
    L, prec = lib_of(layout)
    M, d = x32.shape[0], x32.shape[1] // 2
    src = Rows(x32, layout, 1)
    out = Rows(None, layout, 1, SENTINEL, M, d) if out is None else out
    hip.check(L.cn_op_glu(prec, src.ptr, out.ptr, M, d, hip.current_stream()), "cn_op_glu", L)
    torch.cuda.synchronize()
    return out


def run_dwconv(layout, x, w32, b32, B, L_, k, form):
    """x: float32 (B L, d) or Rows already on the device -> float32 (B L, d) on the host."""
    L, prec = lib_of(layout)
    src = x if isinstance(x, Rows) else Rows(x, layout, k)
    d = w32.shape[0]
    w, b = Vec(w32), Vec(b32)
    y = Rows(None, "fp32", k, SENTINEL, B * L_, d)
    hip.check(L.cn_op_dwconv(prec, src.ptr, w.ptr, b.ptr, y.ptr, B, L_, d, k, form, hip.current_stream()), "cn_op_dwconv", L)
    torch.cuda.synchronize()
    return y


def run_gn(layout, x, gw32, gb32, B, L_, eps=cm.GN_EPS):
    """x: float32 (B L, d) or Rows (fp32) on the device -> (Rows of the output, stats (B, 2) float64 on the host)."""
    L, prec = lib_of(layout)
    src = x if isinstance(x, Rows) else Rows(x, "fp32", 1)
    d = gw32.numel()
    gw, gb = Vec(gw32), Vec(gb32)
    stats = Vec(torch.zeros(2 * B, dtype=torch.float64), fill=-SENTINEL)
    out = Rows(None, layout, 1, SENTINEL, B * L_, d)
    hip.check(L.cn_op_groupnorm_swish(prec, src.ptr, stats.ptr, gw.ptr, gb.ptr, out.ptr, B, L_, d, eps, hip.current_stream()),
              "cn_op_groupnorm_swish", L)
    torch.cuda.synchronize()
    return out, stats.value().reshape(B, 2)


def check(kernel, layout, form, got, ref, bound, what):
    """|got - model| <= bound on every element; prints the figure first and records the worst ratio."""
    err = (got.double() - ref).abs()
    finite = bool(torch.isfinite(got).all())
    ratio = float((err / bound).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    print(f"{kernel} {layout} {form} {what}: worst |err| {float(err.nan_to_num(nan=float('inf')).max()):.2e} = {ratio:.3f} of the bound")
    assert finite, f"{kernel} {layout} {form} {what}: non-finite output (a guard element was read?)"
    if not (err <= bound).all():
        idx = tuple(int(i) for i in torch.unravel_index((err - bound).argmax(), err.shape))
        raise AssertionError(f"{kernel} {layout} {form} {what}: |err| {float(err[idx]):.3e} > bound {float(bound[idx]):.3e} at {idx}; got "
                             f"{float(got[idx]):.9g}, fp64 {float(ref[idx]):.9g}; {int((err > bound).sum())} elements out of bound")
    WORST[(kernel, layout, form)] = max(WORST.get((kernel, layout, form), (0.0, 0.0)), (ratio, float(err.max())))


# ============================================================================================ GLU
@pytest.mark.parametrize("layout,M,d", [(n, M, d) for M, d in cm.GLU_SHAPES for n in layouts_for(d)])
def test_glu(layout, M, d):
    """Saturated gates (+-30), gates whose exponential overflows or vanishes (+-100), exact zeros; split-bf16: the gate at column d + c of a
    2 d wide split row."""
    x32 = cm.glu_case(M, d)
    ref, bound = cm.glu_model(to_layout(x32, layout, device="cpu")[1], layout)
    got, _ = run_glu(layout, x32).value()
    check("glu", layout, "-", got, ref, bound, f"M {M} d {d}")


# ============================================================================================ depthwise convolution
def form_name(k, form):
    return "tiled" if form == 0 and k in cm.DW_TILED_K else "naive"


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("k", cm.DW_TILED_K + cm.DW_NAIVE_K)
def test_dwconv(layout, k):
    """Three differently scaled utterances on one flat buffer: L of 1, below, at and above the halo (k - 1) / 2, at and one past a multiple of
    the 32-frame tile, d beyond one block of 256 channels.  The tiled form equals the naive one bit for bit (k = 3, 7, 15, 31), and each
    utterance run alone equals its rows of the batch bit for bit."""
    B = cm.DW_B
    pad = (k - 1) // 2
    for L_, d in cm.dw_shapes(k):
        if layout == "bf16x3" and not cm.splits(d):
            continue
        x32, w32, b32, _, _, _, ref, bound = cm.dw_reference(layout, k, L_, d)
        src = Rows(x32, layout, k)
        forms = (0, 1) if k in cm.DW_TILED_K else (0,)
        raw = {}
        for form in forms:
            got, raw[form] = run_dwconv(layout, src, w32, b32, B, L_, k, form).value()
            check("dwconv", layout, form_name(k, form), got, ref, bound, f"k {k} L {L_} d {d}")
        if len(forms) == 2:
            assert torch.equal(raw[0], raw[1]), f"{layout} k {k} L {L_} d {d}: the tiled form differs from the naive one"
        if d in (32, 288) and L_ in (1, pad + 1, 33, 97):
            for form in forms:
                for b in range(B):
                    _, alone = run_dwconv(layout, x32[b * L_:(b + 1) * L_], w32, b32, 1, L_, k, form).value()
                    assert torch.equal(alone, raw[form][b * L_:(b + 1) * L_]), (layout, k, L_, d, form, b)


# ============================================================================================ GroupNorm + Swish
@pytest.mark.parametrize("layout,i", [(n, i) for i, ((_, _, d), _) in enumerate(cm.GN_SHAPES) for n in layouts_for(d)])
def test_groupnorm_swish(layout, i):
    """n = L d below, at and above the 1024 threads of the statistics workgroup, no multiple of 64, 64 000 and 512 000; every utterance its
    own mean and scale (mean 32 at std 0.5: the float32 rounding of the mean is the visible part of the bound; a constant image: variance
    0, output swish(beta[c]); a variance below eps).  The sums against correctly rounded ones; each utterance alone bit for bit."""
    (B, L_, d), kinds = cm.GN_SHAPES[i]
    x32, gw32, gb32, x, gw, gb, exact = cm.gn_reference(i)
    ref, bound, _, stats_bound = cm.groupnorm_swish_model(x, gw, gb, B, L_, cm.GN_EPS, layout, stats=exact)
    out, stats = run_gn(layout, x32, gw32, gb32, B, L_)
    check("gn_stats", "-", "-", stats, exact, stats_bound, f"B {B} L {L_} d {d}")
    got, raw = out.value()
    check("gn_swish", layout, "-", got, ref, bound, f"B {B} L {L_} d {d} {kinds}")
    for b, kind in enumerate(kinds):
        rows = slice(b * L_, (b + 1) * L_)
        if kind == "const":
            sw = (gb * torch.sigmoid(gb))[None].expand(L_, d)
            assert ((got[rows] - sw).abs() <= bound[rows]).all(), "zero variance: the output is swish(beta[c])"
        if B > 1:
            out1, stats1 = run_gn(layout, x32[rows], gw32, gb32, 1, L_)
            assert torch.equal(out1.value()[1], raw[rows]), (layout, i, b)
            assert torch.equal(bits(stats1), bits(stats[b:b + 1])), (layout, i, b)


# ============================================================================================ the three in sequence
@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_sequence(layout):
    """GLU -> depthwise convolution -> GroupNorm + Swish on device buffers, as run_conv_module chains them, against the composed models with
    every stage's bound carried into the next."""
    B, L_, d, k = (cm.SEQ_SHAPE[n] for n in ("B", "L", "d", "k"))
    x32, w32, b32, gw32, gb32 = cm.seq_case()
    ref, bound = cm.conv_module_model(to_layout(x32, layout, device="cpu")[1], w32.double(), b32.double(), gw32.double(), gb32.double(), B, L_, k,
                                      cm.GN_EPS, layout)
    glu_out = run_glu(layout, x32, out=Rows(None, layout, k, NAN, B * L_, d))  # (the convolution's NaN guard rows around the GLU's output)
    glu_out.value()
    y = run_dwconv(layout, glu_out, w32, b32, B, L_, k, 0)
    y.value()
    out, _ = run_gn(layout, y, gw32, gb32, B, L_)
    got, _ = out.value()
    check("sequence", layout, "-", got, ref, bound, f"B {B} L {L_} d {d} k {k}")
