"""A float64 model of one launch of the tiled GEMM (csrc/gemm.hip) with a per-element error bound, the buffers of every launch form
the engine uses, and the checks a launch must pass.  Shared by the kernel test (test_gpu_gemm.py), the CPU test that shows the
checks would catch what a kernel can get wrong (test_gemm_model.py) and the argument test (test_gemm_args.py).

The operation (include/cassnat_hip.h, cn_gemm_desc):

    v = (A . W^T) * deq + bias;  ReLU;  Swish;  v * scale + pe[m % period];  resid + resid_scale * v;  v * c_scale (e4m3 output);
    C = the output's rounding of v (e4m3 saturates at +-448)

on the operand VALUES as the kernel receives them: A and W are already in the operand type (fp32, bf16 / fp16, split-bf16 hi + lo,
e4m3), so the model rounds no operand.  What the kernel adds - fp32 accumulation on the matrix cores, one fp32 rounding per
epilogue operation, the output's rounding - is not replayed by the model: the bound covers it.

Two checks per launch (check_launch), no live element exempt from either:

* |out - fp64| <= bound for every live element: 2 gamma(K) sum |a| |w| deq (the factor 2 for what an MFMA's internal adder may do
  differently from K roundings; for e4m3 operands the measured E4M3_ACC instead, below), 2^-18 sum |a| |w| for the lo . lo term the
  split-bf16 product drops, one fp32 rounding per epilogue operation, the incoming bound carried through Swish with Lipschitz
  constant 1.1 plus chain_model.py's term for __expf and the reciprocal, half an output ulp.  A split-bf16 output's halves are
  checked separately: hi against bf16(v), lo against bf16(v - hi) with the hi that was stored.
* the aggregate check: the RMS of (out - fp64) over the live elements within RATIO[layout] of the yardstick
  sqrt(rms(emulation - fp64)^2 + rms(fp32 accumulation)^2).  The emulation is the same operation with float64 accumulation and
  the output's rounding applied (split-bf16 operands: the three-product form hi.hi + hi.lo + lo.hi); the second term is
  chain_model.py's random-walk estimate EPS sqrt(K) (|v| + rms of the row's products + |bias|) carried through the epilogue's
  factors.  The yardstick is never a second launch.

And: what the launch does not own comes back bit for bit - C's columns N .. ldc, its rows past M, the guard regions around every
buffer (a sentinel on the output side); NaN sits in A's rows past M and columns K .. lda, resid's columns N .. ldr, pe's rows past
the period and around every input, so that one read of them shows in the result.
"""
import math

import numpy as np
import torch

from attention_model import EPS, gamma, out_ulp
from attention_model import LAYOUTS as _ATTENTION_LAYOUTS
from cassnat_asr_public_amd import abi

_K = abi.CONSTANTS
RELU, RESID, EMBED, SWISH = (_K["CN_GEMM_EPI_" + n] for n in ("RELU", "RESID", "EMBED", "SWISH"))
OUT = {"own": _K["CN_GEMM_OUT_OWN"], "f32": _K["CN_GEMM_OUT_F32"], "e4m3": _K["CN_GEMM_OUT_E4M3"]}
TILE = {"none": _K["CN_GEMM_TILE_NONE"], "128": _K["CN_GEMM_TILE_128"], "64": _K["CN_GEMM_TILE_64"],
        "fullk": _K["CN_GEMM_TILE_64_FULLK"], "linear256": _K["CN_GEMM_TILE_LINEAR256"]}
ELEM = {"fp32": _K["CN_GEMM_ELEM_F32"], "bf16": _K["CN_GEMM_ELEM_16"], "fp16": _K["CN_GEMM_ELEM_16"],
        "bf16x3": _K["CN_GEMM_ELEM_SPLIT"], "e4m3": _K["CN_GEMM_ELEM_E4M3"]}

# name: (library flavour, CN_PRECISION_*, operand name the library must report); e4m3 operands are the bf16 library's
LAYOUTS = dict(_ATTENTION_LAYOUTS, e4m3=(None, _K["CN_PRECISION_BF16"], "bf16"))
GENERIC = ("fp32", "bf16", "fp16", "bf16x3")
SLAB = {"fp32": 32, "bf16": 64, "fp16": 64, "bf16x3": 32, "e4m3": 128}  # elements of K per 128-byte slab
STORE = {"fp32": "f32", "bf16": "bf16", "fp16": "fp16", "bf16x3": "split", "e4m3": "e4m3"}  # the operand's storage kind
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16, "split": torch.bfloat16, "e4m3": torch.float8_e4m3fn}
INTS = {4: torch.int32, 2: torch.int16, 1: torch.uint8}
E4M3_MAX = 448.0
SENTINEL = 7.0
NAN = float("nan")
GUARD = 64  # elements in front of and behind every buffer (keeps 16-byte alignment in every storage kind)
SWISH_LIP = 1.1
A_SCALE = 16.0  # the e4m3 activations' scale (a power of two, like FP8_S_LN)

# ---- the accumulation term of e4m3 operands.  The matrix core's sum of an e4m3 MFMA's products is not a chain of fp32 adds, so
# the term is measured, not derived: the worst (|out - fp64| - every other term of the bound) / (sum |a| |w| deq) over the e4m3
# cases on the MI355X (for an fp32 output that is |out - fp64| but for a few fp32 roundings; behind a 16-bit or e4m3 rounding only
# the excess over half a step is the accumulation's), then doubled.  Measured 1.343e-5 (f8-big-out-proj, K = 384, fp32 output;
# 1.24e-5 at K = 128, 9.5e-6 at K = 256, 2.2e-6 at K = 2048: it falls with K, the sum of magnitudes grows faster than the
# error), doubled 2.7e-5.  The term may not exceed what test_gemm_fp8_matches_an_e4m3_emulation allows, 1e-4 of the output range
# (max |A . W^T deq + bias| of the launch): it is capped there.  The cap binds in the two K = 2048 cases, where 2.7e-5 sum |a| |w|
# is 1.1 .. 1.5 times that allowance - the constant is set by the shallow products - and the measured error 0.08 .. 0.12 of it.
# docs/KERNEL_NOTES.md holds the numbers.
E4M3_ACC_MEASURED = 1.343e-5
E4M3_ACC = 2.7e-5
E4M3_RANGE_CAP = 1e-4

# ---- what the aggregate check allows: RMS(result - fp64) / yardstick per layout.  Measured on the MI355X over every case of
# CASES (the table in docs/KERNEL_NOTES.md, "Generic GEMM and fused feed-forward: float64 tests of every launch form"), worst:
#   fp32 0.159 (the yardstick's random-walk term over-estimates the matrix core's fp32 accumulation: nothing else is in it);
#   bf16 1.0000, fp16 1.0000 (the error of a 16-bit output IS its rounding; with an fp32 output 0.04 .. 0.06);
#   bf16x3 0.971; e4m3 5.95 (fp32 outputs: the yardstick's fp32 random walk knows nothing of the e4m3 MFMA's own summation;
#   16-bit and e4m3 outputs 1.0000).
# Each value leaves a factor of at least 1.2 above its measurement and sits below the smallest ratio a listed mistake produces
# (test_gemm_model.py prints them: fp32 16466, bf16 113, fp16 1105, bf16x3 198, e4m3 8.3 - no bias behind a saturating e4m3
# output, which the per-element bound catches first).
RATIO = {"fp32": 0.25, "bf16": 1.2, "fp16": 1.2, "bf16x3": 1.2, "e4m3": 7.2}

MISTAKES = ("no_bias", "swish_as_relu", "relu_after_resid", "scale_on_pe", "pe_unwrapped", "resid_scale_ignored", "ldr_as_n",
            "lda_as_k", "ldc_as_n", "last_slab_dropped", "fullk_slab3_dropped", "rows_past_m_stored", "cols_past_n_stored",
            "xcd_tiles_swapped", "w_inv_ignored", "c_scale_before_resid", "no_saturation", "split_lo_dropped_in",
            "split_lo_wrong_offset")


# ================================================================================================ storage
def bits(t):
    return t.contiguous().view(INTS[t.element_size()])


def units(kind):
    """Storage units per element: a split-bf16 element is a bf16 hi and a bf16 lo."""
    return 2 if kind == "split" else 1


def filled(n_elems, kind, value):
    return torch.full((n_elems * units(kind),), value, dtype=torch.float32).to(TORCH[kind])


def index(M, N, ld, kind):
    """Unit index of element (m, n) of a row-major matrix of row stride ld elements, behind the guard: (hi or only, lo or None).
    A split-bf16 row is groups of 32 elements, each 32 hi halves then 32 lo halves (common.h: cn_split_off)."""
    m, n = np.arange(M, dtype=np.int64)[:, None], np.arange(N, dtype=np.int64)[None, :]
    if kind != "split":
        return torch.from_numpy(GUARD + m * ld + n), None
    hi = torch.from_numpy(GUARD * 2 + m * 2 * ld + (n >> 5) * 64 + (n & 31))
    return hi, hi + 32


def read(buf, idx):
    """float64 values at a unit index (through the bits: indexing is not implemented for every storage type)."""
    return bits(buf)[idx].view(buf.dtype).float().double()


def read_elems(buf, M, N, ld, kind):
    hi, lo = index(M, N, ld, kind)
    return (read(buf, hi), read(buf, lo)) if lo is not None else (read(buf, hi), None)


def write(buf, idx, values):
    bits(buf)[idx.reshape(-1)] = bits(values.reshape(-1).to(buf.dtype) if values.dtype != buf.dtype else values.reshape(-1))


def to_e4m3(t):
    return t.float().clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)


def e4m3_ulp(x):
    """One step of e4m3fn at |x| (3 mantissa bits; subnormal step 2^-9), float64."""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -6, max=E4M3_MAX)))
    return 2.0 ** (e - 3)


def out_kind(c, layout):
    """The storage kind of C."""
    if c["out"] == "f32":
        return "f32"
    if c["out"] == "e4m3":
        return "e4m3"
    return "bf16" if layout == "e4m3" else STORE[layout]


def round_out(v, kind):
    """float64 v -> the stored value(s) after the kernel's conversion from fp32: (tensor of the storage type, lo tensor or None)."""
    v32 = v.float()
    if kind == "split":
        hi = v32.to(torch.bfloat16)
        return hi, (v32 - hi.float()).to(torch.bfloat16)
    if kind == "e4m3":
        return to_e4m3(v32), None
    return v32.to(TORCH[kind]), None


def half_ulp(ref, dv, kind):
    """Half a step of the output type at |ref| + dv."""
    a = ref.abs() + dv
    if kind == "f32":
        return torch.zeros_like(ref)
    if kind == "e4m3":
        return 0.5 * e4m3_ulp(a)
    if kind == "split":
        return 0.5 * out_ulp(a, "bf16")
    return 0.5 * out_ulp(a, "bf16" if kind == "bf16" else "fp16")


# ================================================================================================ cases
def case(name, site, M, N, slabs=None, K=None, layouts=GENERIC, out="own", tile="64", bias=True, epi=0, resid=None, ldr_pad=0,
         lda_pad=0, ldc_pad=0, ldc_mul=1, pe=False, period=1, scale=1.0, resid_scale=1.0, c_scale=1.0, w_inv=False, sat=False):
    """One launch.  slabs: K in 128-byte slabs of the layout (K: in elements, for every layout); tile: the form the case is written
    for ("64", "fullk", "128"); resid: None / "inplace" (C is the fp32 residual stream: ldr == ldc) / "sep" (its own buffer of row
    stride N + ldr_pad); ldc = ldc_mul * N + ldc_pad (a split-bf16 output: rounded up to a multiple of 32); pe: EMBED reads a
    table of `period` rows (False with EMBED: scale only); sat: a few planted rows of A that saturate an e4m3 output."""
    assert (slabs is None) != (K is None) and tile in ("64", "fullk", "128") and resid in (None, "inplace", "sep")
    assert (resid is not None) == bool(epi & RESID) and (resid != "inplace" or out == "f32") and (not pe or epi & EMBED)
    return dict(name=name, site=site, M=M, N=N, slabs=slabs, K=K, layouts=tuple(layouts), out=out, tile=tile, bias=bias, epi=epi,
                resid=resid, ldr_pad=ldr_pad, lda_pad=lda_pad, ldc_pad=ldc_pad, ldc_mul=ldc_mul, pe=pe, period=period, scale=scale,
                resid_scale=resid_scale, c_scale=c_scale, w_inv=w_inv, sat=sat)


BIG_M, BIG_N = 3841, 2049  # 31 x 17 = 527 tiles of 128 x 128: the XCD permutation has a remainder of 7; one live row / column last


def _cases():
    out = []
    add = lambda *a, **k: out.append(case(*a, **k))
    # ---- small tile: every ragged edge of M and N (one live row, one live column), slab counts 1 .. 5 and a deep K; 4 slabs is FULLK
    add("shape-M1-N1-s1", "64 x 64", 1, 1, slabs=1)
    add("shape-M63-N33-s2", "64 x 64", 63, 33, slabs=2)
    add("shape-M64-N64-s3-f32", "64 x 64", 64, 64, slabs=3, out="f32")
    add("shape-M65-N65-s5", "64 x 64", 65, 65, slabs=5, ldc_pad=32)
    add("shape-M129-N1-s2-f32", "64 x 64", 129, 1, slabs=2, out="f32", lda_pad=64)
    add("shape-M1-N200-k2048-f32", "64 x 64 deep K", 1, 200, K=2048, out="f32")
    add("shape-M129-N200-s3", "64 x 64", 129, 200, slabs=3, lda_pad=64)
    add("fullk-M65-N65", "64 x 64 FULLK", 65, 65, slabs=4, tile="fullk")
    add("fullk-M129-N200-padded", "64 x 64 FULLK lda > K ldc > N", 129, 200, slabs=4, tile="fullk", lda_pad=64, ldc_pad=32)
    add("fullk-M129-N200-padded-f32", "64 x 64 FULLK lda > K ldc > N", 129, 200, slabs=4, tile="fullk", out="f32", lda_pad=64, ldc_pad=32)
    # ---- big tile: one case per (element type, output type); the fp32-output one has 4 slabs (the big tile takes the loop) and
    # is the residual stream in place
    add("big-own-s3", "128 x 128", BIG_M, BIG_N, slabs=3, tile="128", ldc_pad=31)
    add("big-f32-s4-resid", "128 x 128 out_proj_resid", BIG_M, BIG_N, slabs=4, tile="128", out="f32", ldc_pad=31, epi=RESID,
        resid="inplace")
    # ---- epilogues: every combination a call site passes (bias and pe of unit scale, scale 16, resid_scale 0.5)
    add("epi-none", "no bias", 65, 65, slabs=2, bias=False)
    add("epi-qkv", "run_linear qkv_proj: Q|K|V into a 3 d buffer", 65, 192, slabs=2, lda_pad=64, ldc_mul=3)
    add("epi-relu", "run_linear ffn_w1_relu", 65, 200, slabs=2, epi=RELU)
    add("epi-swish", "run_ffn_swish ffn_w1_swish", 65, 200, slabs=2, epi=SWISH)
    add("epi-resid-inplace", "run_linear out_proj_resid", 65, 65, slabs=2, out="f32", epi=RESID, resid="inplace", ldc_pad=7)
    add("epi-resid-sep", "RESID from a separate buffer, ldr > N", 65, 65, slabs=2, epi=RESID, resid="sep", ldr_pad=5)
    add("epi-macaron", "run_ffn_swish ffn_w2_resid (resid_scale 0.5)", 65, 65, slabs=3, out="f32", epi=RESID, resid="inplace",
        resid_scale=0.5)
    add("epi-embed-pe", "linear_out: EMBED, period 37", 129, 200, slabs=2, out="f32", epi=EMBED, pe=True, period=37, scale=16.0)
    add("epi-embed-scale", "EMBED without pe (scale only)", 65, 65, slabs=2, out="f32", epi=EMBED, scale=16.0)
    add("epi-relu-resid", "ReLU then RESID (the order)", 65, 65, slabs=2, out="f32", epi=RELU | RESID, resid="sep", ldr_pad=3,
        resid_scale=0.5)
    # ---- e4m3 operands: the four call sites of run_enc_layer_fp8, with the weight's scale folded into acc_scale (w_inv_scale
    # null) and on the device; both tiles; K 128, 256, 2048
    E = ("e4m3",)
    for w_inv in (False, True):
        tag = "-winv" if w_inv else ""
        add("f8-qkv-k128" + tag, "run_enc_layer_fp8 qkv_proj_fp8", 129, 192, K=128, layouts=E, ldc_mul=3, w_inv=w_inv)
        add("f8-out-proj-k256" + tag, "run_enc_layer_fp8 out_proj_fp8", 129, 200, K=256, layouts=E, out="f32", epi=RESID,
            resid="inplace", w_inv=w_inv)
        add("f8-ffn-w1-k256" + tag, "run_enc_layer_fp8 ffn_w1_fp8", 129, 200, K=256, layouts=E, out="e4m3", epi=RELU, c_scale=8.0,
            sat=True, w_inv=w_inv)
        add("f8-ffn-w2-k2048" + tag, "run_enc_layer_fp8 ffn_w2_fp8", 65, 65, K=2048, layouts=E, out="f32", epi=RESID,
            resid="inplace", w_inv=w_inv)
    add("f8-big-qkv", "128 x 128 qkv_proj_fp8", BIG_M, BIG_N, K=384, layouts=E, tile="128", ldc_pad=31)
    add("f8-big-out-proj", "128 x 128 out_proj_fp8", BIG_M, BIG_N, K=384, layouts=E, tile="128", out="f32", epi=RESID, resid="inplace",
        ldc_pad=31, w_inv=True)
    add("f8-big-ffn-w1", "128 x 128 ffn_w1_fp8", BIG_M, BIG_N, K=384, layouts=E, tile="128", out="e4m3", epi=RELU, c_scale=8.0, sat=True,
        ldc_pad=31)
    add("f8-e4m3-resid", "e4m3 output behind RESID (the order of c_scale)", 65, 65, K=128, layouts=E, out="e4m3", epi=RESID, resid="sep",
        ldr_pad=3, c_scale=8.0, w_inv=True)
    return out


CASES = _cases()
PAIRS = [(c, layout) for c in CASES for layout in c["layouts"]]


def pair_id(c, layout):
    return f"{c['name']}@{c['site']}@{layout}".replace(" ", "_")


def geometry(c, layout):
    """dict(K, lda, ldc, ldr, okind) of the case in the layout."""
    K = c["K"] if c["K"] is not None else c["slabs"] * SLAB[layout]
    ok = out_kind(c, layout)
    ldc = c["ldc_mul"] * c["N"] + c["ldc_pad"]
    if ok == "split":
        ldc = -(-ldc // 32) * 32
    ldr = ldc if c["resid"] == "inplace" else c["N"] + c["ldr_pad"]
    return dict(K=K, lda=K + c["lda_pad"], ldc=ldc, ldr=ldr, okind=ok)


def tile_edge(c):
    return 128 if c["tile"] == "128" else 64


def form_code(c, layout):
    """The value cn_gemm_form must give for the case: elem | out << 4 | tile << 8."""
    return ELEM[layout] | OUT[c["out"]] << 4 | TILE[c["tile"]] << 8


def descriptor(c, layout, address, acc_scale=1.0):
    """The cn_gemm_desc of the case.  address(name): the device address of buffer `name` (A, W, bias, resid, pe, w_inv, C) behind its
    guard; it is asked only for the buffers the launch has."""
    from cassnat_asr_public_amd import hip

    g = geometry(c, layout)
    resid = None if not c["resid"] else address("C" if c["resid"] == "inplace" else "resid")
    return hip.CnGemmDesc(
        precision=LAYOUTS[layout][1], c_kind=OUT[c["out"]], A=address("A"), W=address("W"), bias=address("bias") if c["bias"] else None,
        C=address("C"), resid=resid, pe=address("pe") if c["pe"] else None, w_inv_scale=address("w_inv") if c["w_inv"] else None,
        lda=g["lda"], ldc=g["ldc"], ldr=g["ldr"] if c["resid"] else 0, M=c["M"], N=c["N"], K=g["K"], epi=c["epi"],
        pe_period=c["period"], resid_scale=c["resid_scale"], scale=c["scale"], ab_fp8=int(layout == "e4m3"), acc_scale=acc_scale,
        c_scale=c["c_scale"], reserved=0)


# ================================================================================================ buffers of a launch
def buffers(c, layout):
    """Host buffers of the launch as the kernel reads and writes them: flat tensors A, W (operand storage), bias, resid, pe, w_inv
    (float32; None where the launch has none; resid None when in place), C.  Every buffer has GUARD elements in front and behind;
    NaN fills whatever the launch must not read, SENTINEL (NaN for the in-place residual stream) what it must not write."""
    g = geometry(c, layout)
    M, N, K = c["M"], c["N"], g["K"]
    kind = STORE[layout]
    rnd = torch.Generator().manual_seed(sum(map(ord, c["name"])) * 131 + ELEM[layout] * 7 + (layout == "fp16"))
    rn = lambda *s: torch.randn(*s, generator=rnd)
    A, W = rn(M, K), rn(N, K) / math.sqrt(K)
    b = dict(w_inv=None, acc_scale=1.0)
    if c["sat"]:  # rows whose products with a few weight rows are far past 448 / c_scale
        for i, r in enumerate(sorted({0, M // 2, M - 1})):
            A[r] = 27.0 * torch.sign(W[(5 * i) % N])
    if layout == "e4m3":
        ws = 2.0 ** math.floor(math.log2(E4M3_MAX / float(W.abs().max())))
        A, W = A * A_SCALE, W * ws
        b["acc_scale"] = 1.0 / A_SCALE if c["w_inv"] else 1.0 / (A_SCALE * ws)
        if c["w_inv"]:
            b["w_inv"] = filled(1 + 2 * GUARD, "f32", NAN)
            b["w_inv"][GUARD] = 1.0 / ws

    def operand(x, rows_alloc, ld):
        buf = filled(2 * GUARD + rows_alloc * ld, kind, NAN)
        hi, lo = index(x.shape[0], x.shape[1], ld, kind)
        if kind == "split":
            h = x.to(torch.bfloat16)
            write(buf, hi, h)
            write(buf, lo, (x - h.float()).to(torch.bfloat16))
        else:
            write(buf, hi, to_e4m3(x) if kind == "e4m3" else x.to(TORCH[kind]))
        return buf

    b["A"] = operand(A, M + 2, g["lda"])
    b["W"] = operand(W, N, K)
    b["bias"] = None
    if c["bias"]:
        b["bias"] = filled(N + 2 * GUARD, "f32", NAN)
        b["bias"][GUARD:GUARD + N] = rn(N)
    b["pe"] = None
    if c["pe"]:
        b["pe"] = filled((c["period"] + 2) * N + 2 * GUARD, "f32", NAN)
        b["pe"][GUARD:GUARD + c["period"] * N] = rn(c["period"] * N)
    ok = g["okind"]
    b["resid"] = None
    if c["resid"] == "inplace":
        b["C"] = filled(2 * GUARD + (M + 2) * g["ldc"], ok, NAN)
        write(b["C"], index(M, N, g["ldc"], ok)[0], rn(M, N))
    else:
        b["C"] = filled(2 * GUARD + (M + 2) * g["ldc"], ok, SENTINEL)
        if c["resid"] == "sep":
            b["resid"] = filled(2 * GUARD + (M + 2) * g["ldr"], "f32", NAN)
            write(b["resid"], index(M, N, g["ldr"], "f32")[0], rn(M, N))
    return b


def offset_bytes(buf, kind):
    """Where the kernel's pointer into a buffer points: behind the front guard."""
    return GUARD * units(kind) * buf.element_size()


def operands(c, layout, b, lda=None, ldr=None, pe_unwrapped=False):
    """The float64 values the launch reads from the buffers ``b``: A and W (split-bf16: (hi, lo)), bias, resid, pe rows per output
    row, deq.  lda / ldr / pe_unwrapped: a kernel that takes a stride or a row wrongly (mistakes)."""
    g = geometry(c, layout)
    M, N, K = c["M"], c["N"], g["K"]
    kind = STORE[layout]
    o = dict(A=read_elems(b["A"], M, K, g["lda"] if lda is None else lda, kind), W=read_elems(b["W"], N, K, K, kind))
    o["bias"] = b["bias"][GUARD:GUARD + N].double() if c["bias"] else None
    o["resid"] = None
    if c["resid"]:
        src = b["C"] if c["resid"] == "inplace" else b["resid"]
        o["resid"] = read(src, index(M, N, g["ldr"] if ldr is None else ldr, "f32")[0])
    o["pe"] = None
    if c["pe"]:
        rows = torch.arange(M).clamp(max=c["period"]) if pe_unwrapped else torch.arange(M) % c["period"]
        o["pe"] = b["pe"][GUARD:GUARD + (c["period"] + 2) * N].view(-1, N)[rows].double()
    o["deq"] = 1.0
    if layout == "e4m3":
        o["deq"] = float(np.float32(b["acc_scale"]) * (np.float32(b["w_inv"][GUARD]) if c["w_inv"] else np.float32(1.0)))
    return o


# ================================================================================================ the float64 model
def split_product_bound(S, K):
    """|hi.hi + hi.lo + lo.hi in fp32 - a . w| of split-bf16 operands a = hi + lo, given S = sum |a| |w| over K: three products per
    element pair (2 gamma(3 K), the factor 2 as for every MFMA sum) and the dropped lo . lo (|lo| <= 2^-9 |value|).  Shared with
    x3_model.py."""
    return 2 * gamma(3 * K) * S + 2.0 ** -18 * S


def gemm_model(c, layout, o, mistakes=()):
    """One launch in float64 from the operand values ``o`` (operands()) -> dict(ref, dv, half, emu_v, acc, S): the fp64 result (an
    e4m3 output: saturated), the bound of the kernel's fp32 v in front of the output's rounding, half an output step, the
    emulation's v (float64 accumulation; ``mistakes`` change it and nothing else), the random-walk term, sum |a| |w| deq and the
    e4m3 accumulation term, both times the epilogue's factor (what an error of the product becomes in v)."""
    bad = set(mistakes)
    assert bad <= set(MISTAKES), bad
    g = geometry(c, layout)
    K, ok, epi = g["K"], g["okind"], c["epi"]
    (Ah, Al), (Wh, Wl) = o["A"], o["W"]
    A = Ah if Al is None else Ah + Al
    W = Wh if Wl is None else Wh + Wl
    deq = o["deq"]
    P = (A @ W.T) * deq
    S = (A.abs() @ W.abs().T) * abs(deq)
    f8_term = None
    if layout == "e4m3":                                      # the measured term, capped at the old test's allowance
        rng = (P + (o["bias"] if o["bias"] is not None else 0.0)).abs().max()
        f8_term = torch.minimum(E4M3_ACC * S, E4M3_RANGE_CAP * rng)
        dv = f8_term + 2 * EPS * P.abs()                      # ... and the two multiplications by the scales
    elif layout == "bf16x3":
        dv = split_product_bound(S, K)
    else:
        dv = 2 * gamma(K + 1) * S                             # (fp32 operands: the product's own rounding)
    # ---- the emulation's product
    if layout == "bf16x3":
        if "split_lo_dropped_in" in bad:
            E = Ah @ Wh.T
        else:
            E = Ah @ Wh.T + Ah @ Wl.T + Al @ Wh.T
    else:
        E = A @ W.T
    drop = "last_slab_dropped" in bad or "fullk_slab3_dropped" in bad
    if drop:
        E = E - A[:, K - SLAB[layout]:] @ W[:, K - SLAB[layout]:].T
    E = E * (deq if "w_inv_ignored" not in bad else float(np.float32(o["deq_no_w_inv"])))
    row_rms = lambda t: t.pow(2).mean(-1, keepdim=True).sqrt()
    acc = EPS * math.sqrt(K) * (P.abs() + row_rms(P))
    v = P
    lin = 1.0                                                # the epilogue's factor on an error of the product
    step = lambda v, dv: dv + EPS * (v.abs() + dv)           # one fp32 rounding of the operation's result
    if o["bias"] is not None:
        v = v + o["bias"]
        dv = step(v, dv)
        acc = acc + EPS * math.sqrt(K) * o["bias"].abs()
        if "no_bias" not in bad:
            E = E + o["bias"]
    relu_e = lambda t: torch.relu(t)
    swish = lambda t: t * torch.sigmoid(t)
    if epi & RELU:
        dv = torch.where(v < -dv, torch.zeros_like(dv), dv)    # negative beyond its bound: an exact 0 in the kernel too
        acc = torch.where(v < 0, torch.zeros_like(acc), acc)
        v = torch.relu(v)
        if "relu_after_resid" not in bad:
            E = relu_e(E)
    if epi & SWISH:
        h = swish(v)
        dv = SWISH_LIP * dv + 2 * (4 * v.abs() + 16) * EPS * h.abs() + EPS * h.abs()
        acc = acc * SWISH_LIP
        lin *= SWISH_LIP
        v = h
        E = relu_e(E) if "swish_as_relu" in bad else swish(E)
    if epi & EMBED:
        pe = o["pe"] if o["pe"] is not None else 0.0
        v = v * c["scale"]
        dv = step(v, dv * abs(c["scale"]))
        v = v + pe
        dv = step(v, dv)
        acc = acc * abs(c["scale"])
        lin *= abs(c["scale"])
        E = (E + pe) * c["scale"] if "scale_on_pe" in bad else E * c["scale"] + pe
    if epi & RESID:
        rs = c["resid_scale"]
        v = rs * v
        dv = step(v, dv * abs(rs))
        v = o["resid"] + v
        dv = step(v, dv)
        acc = acc * abs(rs)
        lin *= abs(rs)
        rs_e = 1.0 if "resid_scale_ignored" in bad else rs
        if "c_scale_before_resid" in bad:
            E = o["resid"] + rs_e * E * c["c_scale"]
        else:
            E = o["resid"] + rs_e * E
        if "relu_after_resid" in bad:
            E = relu_e(E)
    if ok == "e4m3":
        v = v * c["c_scale"]
        dv = step(v, dv * c["c_scale"])
        acc = acc * c["c_scale"]
        lin *= c["c_scale"]
        if "c_scale_before_resid" not in bad:
            E = E * c["c_scale"]
        v = v.clamp(-E4M3_MAX, E4M3_MAX)                       # (the clamp is 1-Lipschitz: dv holds behind it)
    return dict(ref=v, dv=dv, half=half_ulp(v, dv, ok), emu_v=E, acc=acc, S=S * lin, f8_term=None if f8_term is None else f8_term * lin)


def emu_value(emu_v, kind, saturate=True):
    """The emulation's stored output as float64 (split-bf16: hi + lo)."""
    if kind == "e4m3" and not saturate:
        return emu_v.float().to(torch.float8_e4m3fn).float().double()  # past 448: NaN
    hi, lo = round_out(emu_v, kind)
    return hi.float().double() + (0 if lo is None else lo.float().double())


_MODEL = {}


def model_of(c, layout, b):
    """gemm_model of the case's own buffers; kept for the cases below a million outputs (the big ones are computed per use)."""
    key = (c["name"], layout)
    if key in _MODEL:
        return _MODEL[key]
    res = gemm_model(c, layout, operands(c, layout, b))
    if c["M"] * c["N"] <= 1 << 20:
        _MODEL[key] = res
    return res


# ================================================================================================ a launch on the CPU
def emulate_launch(c, layout, b, mistakes=()):
    """What a launch leaves in C of the buffers ``b`` (in place), from the emulation: a stand-in for the kernel on the CPU."""
    bad = set(mistakes)
    assert bad <= set(MISTAKES), bad
    g = geometry(c, layout)
    M, N, K, ok = c["M"], c["N"], g["K"], g["okind"]
    o = operands(c, layout, b, lda=K if "lda_as_k" in bad else None, ldr=N if "ldr_as_n" in bad else None,
                 pe_unwrapped="pe_unwrapped" in bad)
    o["deq_no_w_inv"] = b["acc_scale"]
    res = gemm_model(c, layout, o, bad) if bad else model_of(c, layout, b)
    E = res["emu_v"]
    if "xcd_tiles_swapped" in bad:  # the first two tiles along N exchange their places
        t = tile_edge(c)
        w = min(t, N - t)
        E = E.clone()
        E[:t, :w], E[:t, t:t + w] = res["emu_v"][:t, t:t + w], res["emu_v"][:t, :w]
    rows, cols = M, N
    if "rows_past_m_stored" in bad:  # the clamped source row M - 1 once more, stored at row M
        E, rows = torch.cat([E, E[-1:]], 0), M + 1
    if "cols_past_n_stored" in bad:
        E, cols = torch.cat([E, E[:, -1:]], 1), N + 1
    hi_i, lo_i = index(rows, cols, N if "ldc_as_n" in bad else g["ldc"], ok)
    if ok == "e4m3" and "no_saturation" in bad:
        hi, lo = E.float().to(torch.float8_e4m3fn), None
    else:
        hi, lo = round_out(E, ok)
    write(b["C"], hi_i, hi)
    if lo is not None:
        write(b["C"], lo_i + (32 if "split_lo_wrong_offset" in bad else 0), lo)
    return b


class LaunchError(AssertionError):
    """A launch that fails check_launch.  kind: "untouched", "bound" or "ratio"; ratio: the rms ratio of a "ratio" failure."""

    def __init__(self, kind, text, ratio=None):
        super().__init__(text)
        self.kind, self.ratio = kind, ratio


def check_launch(c, layout, before, after, worst=None, enforce=True):
    """The checks of the module's docstring.  ``worst``: a dict that receives bound (worst |err| / bound), rms (the aggregate
    ratio) and, for e4m3 operands, acc (worst (|err| - the rest of the bound) / sum |a| |w| deq: what E4M3_ACC is measured from).
    enforce=False: measure only (the untouched check still raises)."""
    g = geometry(c, layout)
    M, N, ok = c["M"], c["N"], g["okind"]
    hi_i, lo_i = index(M, N, g["ldc"], ok)
    for name in ("A", "W", "bias", "resid", "pe", "w_inv", "C"):
        if not torch.is_tensor(before.get(name)):
            continue
        same = bits(before[name]) == bits(after[name])
        if name == "C":
            same[hi_i.reshape(-1)] = True
            if lo_i is not None:
                same[lo_i.reshape(-1)] = True
        if not bool(same.all()):
            where = int((~same).nonzero()[0])
            raise LaunchError("untouched", f"{layout} {c['name']}: {name}[unit {where}] was written and is not the launch's to write "
                              f"({int((~same).sum())} such units)")
    res = model_of(c, layout, before)
    ref, dv, half = res["ref"], res["dv"], res["half"]
    got_hi = read(after["C"], hi_i)
    rms = lambda t: float(t.pow(2).mean().sqrt())

    def bound_check(what, err, bound, got, want):
        okay = err <= bound
        if enforce and not bool(okay.all()):
            at = tuple(int(v) for v in (~okay).nonzero()[0])
            raise LaunchError("bound", f"{layout} {c['name']} {what}: |err| {float(err[at]):.3e} > bound {float(bound[at]):.3e} at "
                              f"(row, column) = {at}; got {float(got[at]):.6g}, fp64 {float(want[at]):.6g}; {int((~okay).sum())} "
                              "elements out of bound")
        r = err / bound.clamp(min=1e-300)
        return float(torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r).max())

    if lo_i is None:
        got = got_hi
        bratio = bound_check("C", (got - ref).abs(), dv + half, got, ref)
    else:
        got_lo = read(after["C"], lo_i)
        got = got_hi + got_lo
        bratio = bound_check("hi half", (got_hi - ref).abs(), dv + half, got_hi, ref)
        rest = ref - got_hi  # what the lo half has to hold, given the hi half that was stored
        bratio = max(bratio, bound_check("lo half", (got_lo - rest).abs(), dv + 0.5 * out_ulp(rest.abs() + dv, "bf16"), got_lo, rest))
        bratio = max(bratio, bound_check("hi + lo", (got - ref).abs(), dv + 2.0 ** -17 * ref.abs() + 1e-38, got, ref))
    emu = emu_value(res["emu_v"], ok)
    yard = math.sqrt(rms(emu - ref) ** 2 + rms(res["acc"]) ** 2)
    dev = rms(got - ref)
    ratio = dev / yard if yard > 0 else (0.0 if dev == 0 else float("inf"))
    if math.isnan(ratio):
        ratio = float("inf")
    if worst is not None:
        worst["bound"], worst["rms"] = bratio, ratio
        if layout == "e4m3":
            rest = dv - res["f8_term"] + half
            err = (got - ref).abs()  # (an exact result - a ReLU's 0, a saturated 448 - shows no accumulation error)
            worst["acc"] = float((torch.where(err > 0, err - rest, torch.zeros_like(err)).clamp(min=0) / res["S"].clamp(min=1e-300)).max())
    if enforce and not ratio <= RATIO[layout]:
        raise LaunchError("ratio", f"{layout} {c['name']}: rms(result - fp64) {dev:.3e} is {ratio:.2f} x the yardstick {yard:.3e} "
                          f"(emulation {rms(emu - ref):.3e}); allowed {RATIO[layout]}", ratio)
