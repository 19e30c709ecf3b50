"""A float64 model of one launch of the fused generator tail (csrc/genmax.hip) with derived error bounds, an emulation of the
kernel's scheme in numpy, the buffers of every launch form, and the checks a launch must pass.  Shared by the kernel test
(test_gpu_genmax.py), the CPU test that shows the checks catch what a kernel can get wrong (test_genmax_model.py) and the argument
and coverage test (test_genmax_args.py).

The operation (include/cassnat_hip_genmax.h, cn_genmax_desc): per row m < count (count = *m_dev, or M)

    l = W h[m] + b;   arg = the lowest v with l[v] = max l;   maxlp = log_softmax(l)[arg];   tgt_lp = log_softmax(l)[target]

on the operand VALUES the kernel sees: h as stored (bf16, half, or split-bf16 hi + lo), W rounded by the library's pack (the
rounding of cn_host_op16; split-bf16: hi + lo).  The float64 model rounds nothing else; what the kernel adds is covered by bounds:

* per logit  E_v = 2 gamma(K + 1) sum_k |w_vk| |h_k| at K = 256 (gemm_model.py's convention: the factor 2 for what an MFMA's adder
  may do differently from K roundings; split-bf16: gemm_model.split_product_bound, three products and the dropped lo . lo), then
  one fp32 rounding for the bias add.
* arg-max: a row is DECIDED when its float64 top-2 gap exceeds E_top1 + E_top2 - it must match exactly.  On an undecided row the
  index must be a candidate: a v whose float64 logit is within E_v + E_top1 of the maximum.  Vocabulary rows planted as
  bit-identical duplicates count as one entry for the gap, and the lowest of them must be returned.  At most 1 % of a random
  case's rows and none of a planted case's may be undecided (test_genmax_model.py checks that on the model alone).
* maxlp and tgt_lp: |out - fp64| <= min(derived + FAST * unit, CAP).  derived = E of the maximum (the largest E among the
  candidates) or of the target + the softmax-weighted mean of E_v + the summation: every exponential passes through at most
  n = 16 + vtw (the adds of its tile and of the tiles behind it) + vtw (a rescale per tile at most) + 3 (half merge) + 3 (waves - 1)
  (wave merge) roundings of a sum of positive terms, gamma(n) relative to the sum and so absolute in its logarithm; the
  subtraction l - max in front of each exponential, EPS sum p_v |l_v - max|; logf's own rounding EPS |log s|; for the gather the
  two roundings of (l_t - max) - log s.  unit = EPS (1 + sum_v p_v |l_v - max| + |log s|) is what one unit of relative error in
  every fast __expf (whose argument error grows with |l_v - max|) and in logf amounts to; FAST is measured on the MI355X, below.
  CAP is the allowance of the older tests in test_gpu_kernels.py (2e-4 for the 16-bit kernel, 1e-4 for the split one): the total
  never exceeds it.  Where the float64 result is -inf (a target outside [0, V)) the output must be -inf exactly.

And: what the launch does not own comes back bit for bit - rows at or past the count, columns U .. ld of the targets' output, the
guard elements around every buffer, every input.
"""
import math

import numpy as np
import torch

from attention_model import EPS, gamma
from cassnat_asr_public_amd import abi
from gemm_model import split_product_bound

_K, _G = abi.CONSTANTS, abi.GENMAX_CONSTANTS
KINDS = {"lse": _G["CN_GENMAX_KIND_ARGMAX_LSE"], "argmax": _G["CN_GENMAX_KIND_ARGMAX"], "gather": _G["CN_GENMAX_KIND_GATHER"]}
KERNEL_CODE = {"16": _G["CN_GENMAX_KERNEL_16"], "split": _G["CN_GENMAX_KERNEL_SPLIT"]}
# name: (library flavour, CN_PRECISION_*, operand name the library must report, kernel)
LAYOUTS = {"bf16": (None, _K["CN_PRECISION_BF16"], "bf16", "16"), "fp16": ("f16", _K["CN_PRECISION_F16"], "fp16", "16"),
           "bf16x3": (None, _K["CN_PRECISION_BF16X3"], "bf16", "split")}
WAVES = {"16": 4, "split": 8}
D = 256
MAX_V = 6144
GUARD = 64
NEG_FILL = np.float32(np.finfo(np.float32).min)  # CN_NEG_FILL: where a running maximum starts
ARG_SENTINEL, TGT_FILL = -7, -5
NAN16 = 0x7FC0  # a NaN in bf16 and in half

# ---- the measured part of the maxlp / tgt_lp bound: FAST * unit.  Measured on the MI355X as the worst
# (|out - fp64| - derived) / unit over every launch of LAUNCHES (test_gpu_genmax.py prints it with -s); asserted: twice that
# maximum (the precedent of gemm_model.E4M3_ACC), and nothing where the derived part alone covers every launch.
# docs/KERNEL_NOTES.md, "Fused generator tail: float64 tests of every launch form", holds the numbers.
FAST_MEASURED = 0.0
FAST = 2.0 * max(FAST_MEASURED, 0.0)
CAP = {"16": 2e-4, "split": 1e-4}
UNDECIDED_CAP = 0.01

MISTAKES = ("map_r", "half_offset_dropped", "tie_high_fold", "tie_high_half", "tie_high_wave", "no_rescale", "wave_merge_no_rescale",
            "pad_bias_zero", "last_tile_dropped", "no_bias", "maxlp_is_max_logit", "gather_returns_logit", "gather_ld_as_u",
            "m_dev_ignored", "split_no_wlo_xhi", "split_no_whi_xlo", "half_pack_as_bf16")


# ================================================================================================ the kernel's geometry
def vtw_of(kernel, V):
    """32-entry vocabulary tiles per wave (genmax_vtw / genmax_x3_vtw)."""
    tiles = -(-V // 32)
    if kernel == "split":
        return -(-tiles // 8)
    t = -(-tiles // 4)
    return t + (t & 1)


def mt_of(kernel, M):
    """32-row tiles per workgroup (decide_genmax)."""
    if M == 0:
        return 0
    return (2 if M > 32 else 1) if kernel == "16" else (2 if -(-M // 32) > 256 else 1)


def padded_v(kernel, V):
    return 32 * WAVES[kernel] * vtw_of(kernel, V)


def lds_bytes(kernel, mt, vtw):
    w = WAVES[kernel]
    return max(mt * (16384 if kernel == "16" else 32768) + w * vtw * 32 * 4, w * 32 * mt * 16)


def form_code(M, V, layout, kind):
    """The value cn_genmax_form must give: kernel | rows << 4 | kind << 8 | vtw << 12."""
    kernel = LAYOUTS[layout][3]
    return KERNEL_CODE[kernel] | mt_of(kernel, M) << 4 | KINDS[kind] << 8 | vtw_of(kernel, V) << 12


def form_parts(code):
    return code & 15, code >> 4 & 15, code >> 8 & 15, code >> 12


# ================================================================================================ operand rounding and packing
def op16(x32, layout):
    """float32 array -> (the 16 bits of the library's operand as uint16, its value as float32): cn_host_op16."""
    t = torch.from_numpy(np.ascontiguousarray(x32, np.float32)).to(torch.float16 if layout == "fp16" else torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16), t.float().numpy()


def split16(x32):
    """float32 -> hi, lo as (bits, value) pairs: hi = bf16(x), lo = bf16(x - hi)."""
    hb, hv = op16(x32, "bf16")
    lb, lv = op16(np.asarray(x32, np.float32) - hv, "bf16")
    return (hb, hv), (lb, lv)


def pack_model(W, b, V, layout):
    """The packed weight stream and bias table of pack_genmax / pack_genmax_x3 stated in numpy -> (uint16 [waves][vtw][16][(2)][64][8],
    float32 [waves * vtw * 32]): element j of lane l of fragment (wave, tile, ks) is W[32 (wave vtw + tile) + (l & 31)][16 ks + 8 (l >> 5) + j]."""
    kernel = LAYOUTS[layout][3]
    waves, vtw = WAVES[kernel], vtw_of(kernel, V)
    P = 32 * waves * vtw
    lane, j, ks = np.arange(64), np.arange(8), np.arange(16)
    v = (32 * np.arange(waves * vtw)[:, None] + (lane & 31)[None, :])[:, None, :, None]           # [wave tile][1][lane][1]
    k = (16 * ks[:, None, None] + 8 * (lane >> 5)[None, :, None] + j[None, None, :])[None]       # [1][ks][lane][j]
    bias = np.full(P, -np.inf, np.float32)
    bias[:V] = b

    def stream(bits):
        padded = np.zeros((P, D), np.uint16)
        padded[:V] = bits
        return padded[np.broadcast_to(v, (waves * vtw, 16, 64, 8)), np.broadcast_to(k, (waves * vtw, 16, 64, 8))]

    if kernel == "16":
        return stream(op16(W, layout)[0]).reshape(waves, vtw, 16, 64, 8), bias
    (hb, _), (lb, _) = split16(W)
    return np.stack([stream(hb), stream(lb)], axis=2).reshape(waves, vtw, 16, 2, 64, 8), bias


# ================================================================================================ cases
# seeds of the random cases that need another than 0 for the model alone to decide every row (a case of under 100 rows may have no
# undecided row under the 1 % cap; test_genmax_model.py checks the cap)
SEEDS = {"shape-M97-V384": 1, "shape-M97-V1028": 1, "shape-M65-V257": 2, "shape-M65-V6144": 2, "mdev-70-of-96": 2, "mdev-0-of-96": 1,
         "mdev-1-of-66": 1, "halfneg-V1028": 1}


def case(name, M, V, layouts, data="random", U=1, ld=1, count=None, modes=("mixed",), kinds=("lse", "argmax", "gather"), seed=None):
    """One set of inputs, launched once per output kind (the gather once per target mode).  data: how h, W and b are planted;
    U, ld: the gather's row map (M % U == 0); count: the value of *m_dev (None: no m_dev)."""
    assert M % U == 0 and ld >= U
    seed = SEEDS.get(name, 0) if seed is None else seed
    return dict(name=name, M=M, V=V, layouts=tuple(layouts), data=data, U=U, ld=ld, count=count, modes=tuple(modes), kinds=tuple(kinds),
                seed=seed)


UL = {1: (1, 1), 31: (31, 33), 32: (8, 8), 33: (11, 13), 63: (9, 12), 64: (16, 17), 65: (5, 7), 97: (1, 3)}  # M: (U, ld)
K16, KX3 = ("bf16", "fp16"), ("bf16x3",)
WINS = ("winner", "last", "zero", "other")


def _cases():
    out = []
    add = lambda *a, **k: out.append(case(*a, **k))
    # ---- 16-bit kernel: every M around the MT threshold at two vocabularies, every V at three row counts
    pairs = [(M, V) for M in (1, 31, 32, 33, 63, 64, 65, 97) for V in (384, 1028)] + [(M, V) for M in (1, 33, 97) for V in (40, 4234, 6144)]
    for M, V in pairs:
        add(f"shape-M{M}-V{V}", M, V, K16, U=UL[M][0], ld=UL[M][1])
    # ---- split kernel: every V at small M; the wide form once
    for V in (1, 257, 1028, 6144):
        for M in (1, 33, 65):
            add(f"shape-M{M}-V{V}", M, V, KX3, U=UL[M][0], ld=UL[M][1])
    add("wide-M8225-V257", 8225, 257, KX3, U=7, ld=9)
    # ---- the device-side row count: across a workgroup boundary, on one, equal to M, 1, and 0 (every workgroup leaves at once)
    for count in (70, 64, 96, 1, 0):
        add(f"mdev-{count}-of-96", 96, 384, K16, U=8, ld=9, count=count)
    for count in (40, 32, 66, 1, 0):
        add(f"mdev-{count}-of-66", 66, 257, KX3, U=6, ld=8, count=count)
    # ---- planted: every entry wins one row
    add("wins-V384", 384, 384, K16, data="wins", U=6, ld=7, modes=WINS)
    add("wins-V1028", 1028, 1028, K16, data="wins", U=4, ld=4, modes=WINS)
    add("wins-V257", 257, 257, KX3, data="wins", U=1, ld=2, modes=WINS)
    # ---- planted: bit-identical duplicates of the winner one entry, one lane half, one tile, one wave away and at V - 1
    add("dups-V1028", 40, 1028, K16 + KX3, data="dups", U=8, ld=9, modes=("winner",))
    # ---- what the log-sum-exp sees
    for data in ("peaked", "flat", "offset", "halfneg", "spiky"):
        add(f"{data}-V1028", 33, 1028, K16 + KX3, data=data, U=11, ld=13)
    add("flat-V384", 65, 384, K16, data="flat", U=5, ld=7)
    add("flat-V257", 33, 257, KX3, data="flat", U=11, ld=13)
    return out


CASES = _cases()
BY_NAME = {}
for _c in CASES:
    for _l in _c["layouts"]:
        BY_NAME[(_c["name"], _l)] = _c
# one launch: (case, layout, kind, target mode or None)
LAUNCHES = [(c, layout, kind, mode) for c in CASES for layout in c["layouts"] for kind in c["kinds"]
            for mode in (c["modes"] if kind == "gather" else (None,))]
PLANTED = ("wins", "dups", "peaked", "flat")


def launch_id(c, layout, kind, mode):
    return f"{c['name']}@{layout}@{kind}" + (f"-{mode}" if mode else "")


def dup_deltas(kernel, V):
    """How far above the winner its duplicate sits: the next entry of a lane, the other lane half, the next tile, the next wave."""
    return (1, 4, 32, 32 * vtw_of(kernel, V))


def winner_of(c, layout):
    """Row m's planted winner (wins, peaked, dups), and for dups the index of its duplicate."""
    M, V = c["M"], c["V"]
    m = np.arange(M)
    if c["data"] == "dups":
        deltas = dup_deltas(LAYOUTS[layout][3], V)
        rng = np.random.default_rng(11)
        used, v, dup = {V - 1}, [], []
        for i in range(M):                                 # row i: distance i % 4; the last row's duplicate is V - 1
            d = deltas[i % 4]
            while True:
                a = int(rng.integers(0, V - 1 - deltas[3]))
                b = V - 1 if i == M - 1 else a + d
                # the pair meets where its distance says: one lane's next entry, the other half of one tile, one wave's next tile
                vtw = deltas[3] // 32
                fits = (a % 4 != 3, a % 32 < 28, (a // 32) % vtw != vtw - 1, True)[i % 4]
                if a not in used and (i == M - 1 or (b not in used and fits)):
                    break
            used |= {a, b}
            v.append(a)
            dup.append(b)
        return np.array(v), np.array(dup)
    step = 5 if V % 5 else 7
    return (3 + step * m) % V, None


_RAW = {}


def raw(c, layout):
    """fp32 h [M][256], W [V][256], b [V] of the case and dup_of [V]: the lowest index of each entry's group of bit-identical rows.
    The same for every layout but for dups, whose wave distance is the kernel's."""
    key = (c["name"], LAYOUTS[layout][3] if c["data"] == "dups" else "")
    if key in _RAW:
        return _RAW[key]
    M, V, data = c["M"], c["V"], c["data"]
    rng = np.random.default_rng(1000 * c["seed"] + sum(map(ord, c["name"])))
    W = (rng.standard_normal((V, D)) / 16).astype(np.float32)
    b = (0.1 * rng.standard_normal(V)).astype(np.float32)
    h = rng.standard_normal((M, D)).astype(np.float32)
    dup_of = np.arange(V)
    if data in ("wins", "peaked", "dups"):
        v, dup = winner_of(c, layout)
        if dup is not None:
            W[dup], b[dup], dup_of[dup] = W[v], b[v], v
        scale = 52.0 if data == "peaked" else 16.0       # the winner's logit; the others' spread is scale / 16
        h = (scale * W[v] / (W[v].astype(np.float64) ** 2).sum(-1, keepdims=True)).astype(np.float32)
    elif data == "flat":
        W[:], b[:], dup_of[:] = 0.0, 0.25, 0
    elif data == "offset":
        b += np.float32(60.0)
    elif data == "halfneg":
        b[1::2] = -30.0
    elif data == "spiky":                                 # a few large channels, as a LayerNorm output has
        h[:, [3, 77, 130, 255]] = (30.0 * np.where((np.arange(M)[:, None] + np.arange(4)[None]) % 2, 1.0, -1.0)).astype(np.float32)
    else:
        assert data == "random", data
    _RAW[key] = (h, W, b, dup_of)
    return _RAW[key]


def targets(c, layout, mode):
    """int32 [B][ld]: the gather's targets, TGT_FILL in columns U .. ld."""
    M, V, U, ld = c["M"], c["V"], c["U"], c["ld"]
    kernel = LAYOUTS[layout][3]
    m = np.arange(M)
    if mode == "mixed":
        rng = np.random.default_rng(7 + sum(map(ord, c["name"])))
        t = rng.integers(0, V, M)
        t[0], t[-1] = V - 1, 0
        outside = [-1, V, padded_v(kernel, V) - 1, 2 ** 30]  # (the third is V - 1, a live entry, where the tiles hold no padding)
        sel = m % 5 == 2
        t[sel] = np.array(outside)[(m[sel] // 5) % 4]
    else:
        w = winner_of(c, layout)[0]
        t = {"winner": w, "last": np.full(M, V - 1), "zero": np.zeros(M, np.int64), "other": (w + 1) % V}[mode]
    out = np.full((M // U, ld), TGT_FILL, np.int32)
    out[:, :U] = t.reshape(M // U, U)
    return out


# ================================================================================================ buffers of a launch
def h_storage(h, layout):
    """fp32 [M][256] -> the uint16 rows the kernel reads: 256 operands, or a split-bf16 row of 512 (per 32 columns 32 hi, 32 lo)."""
    if LAYOUTS[layout][3] == "16":
        return op16(h, layout)[0]
    (hb, _), (lb, _) = split16(h)
    return np.stack([hb.reshape(-1, 8, 32), lb.reshape(-1, 8, 32)], axis=2).reshape(-1, 512)


def h_values(rows, layout):
    """uint16 rows as stored -> float64 (hi, lo or None)."""
    dt = torch.float16 if layout == "fp16" else torch.bfloat16
    val = lambda bits: torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(dt).double().numpy()
    if LAYOUTS[layout][3] == "16":
        return val(rows), None
    g = rows.reshape(-1, 8, 2, 32)
    return val(g[:, :, 0, :].reshape(-1, D)), val(g[:, :, 1, :].reshape(-1, D))


def buffers(c, layout, kind, mode):
    """Host buffers of the launch (numpy): h (uint16, M + 2 rows, NaN outside the M rows), W, b (fp32, host operands), arg, maxlp,
    tgt, tgt_lp, m_dev (None where the launch has none).  Every device buffer has GUARD elements in front and behind."""
    M, V = c["M"], c["V"]
    h, W, b, _ = raw(c, layout)
    rows = h_storage(h, layout)
    hb = np.full(2 * GUARD + (M + 2) * rows.shape[1], NAN16, np.uint16)
    hb[GUARD:GUARD + rows.size] = rows.reshape(-1)
    out = dict(h=hb, W=W.copy(), b=b.copy(), arg=None, maxlp=None, tgt=None, tgt_lp=None, m_dev=None)
    if kind == "gather":
        t = targets(c, layout, mode)
        out["tgt"] = np.full(2 * GUARD + t.size, TGT_FILL, np.int32)
        out["tgt"][GUARD:GUARD + t.size] = t.reshape(-1)
        out["tgt_lp"] = np.full(2 * GUARD + t.size, np.nan, np.float32)
    else:
        out["arg"] = np.full(2 * GUARD + M, ARG_SENTINEL, np.int32)
        if kind == "lse":
            out["maxlp"] = np.full(2 * GUARD + M, np.nan, np.float32)
    if c["count"] is not None:
        out["m_dev"] = np.full(2 * GUARD + 1, ARG_SENTINEL, np.int32)
        out["m_dev"][GUARD] = c["count"]
    return out


def copy_of(bufs):
    return {k: (None if v is None else v.copy()) for k, v in bufs.items()}


def descriptor(c, layout, kind, address):
    """The cn_genmax_desc of the launch.  address(name): the address of buffer `name` behind its guard (W and b: host)."""
    from cassnat_asr_public_amd import hip

    gather = kind == "gather"
    return hip.CnGenmaxDesc(
        precision=LAYOUTS[layout][1], reserved=0, h_dev=address("h"), w_host=address("W"), b_host=address("b"), M=c["M"], V=c["V"],
        arg_dev=None if gather else address("arg"), maxlp_dev=address("maxlp") if kind == "lse" else None,
        m_dev=address("m_dev") if c["count"] is not None else None, tgt_dev=address("tgt") if gather else None,
        U=c["U"] if gather else 0, ld=c["ld"] if gather else 0, tgt_lp_dev=address("tgt_lp") if gather else None)


def live_count(c):
    return c["M"] if c["count"] is None else c["count"]


def tgt_index(c, m, ld_as_u=False):
    """Where row m's target and result sit in the [B][ld] buffers."""
    U = c["ld"] if ld_as_u else c["U"]
    return (m // U) * c["ld"] + m % U


# ================================================================================================ the float64 model
def operands(c, layout, bufs, w_layout=None):
    """What the launch reads, float64: h (hi, lo), W (hi, lo) as the library's pack rounds it, b."""
    M = c["M"]
    width = 256 if LAYOUTS[layout][3] == "16" else 512
    hh, hl = h_values(bufs["h"][GUARD:GUARD + M * width].reshape(M, width), layout)
    if LAYOUTS[layout][3] == "16":
        Wh, Wl = op16(bufs["W"], w_layout or layout)[1].astype(np.float64), None
    else:
        (_, hv), (_, lv) = split16(bufs["W"])
        Wh, Wl = hv.astype(np.float64), lv.astype(np.float64)
    return dict(h=(hh, hl), W=(Wh, Wl), b=bufs["b"].astype(np.float64))


_MODEL = {}


def model_of(c, layout, bufs):
    """The float64 results and bounds of the case (kept per case and layout): logits l, E, arg (the lowest index of the maximum's
    group), decided, cand [M][V], maxlp, e_top, mean_e, sum_term, unit."""
    key = (c["name"], layout)
    if key in _MODEL:
        return _MODEL[key]
    kernel = LAYOUTS[layout][3]
    o = operands(c, layout, bufs)
    dup_of = raw(c, layout)[3]
    (hh, hl), (Wh, Wl) = o["h"], o["W"]
    h = hh if hl is None else hh + hl
    W = Wh if Wl is None else Wh + Wl
    S = np.abs(h) @ np.abs(W).T
    l = h @ W.T
    l = l[:, dup_of] + o["b"][dup_of][None]      # a group of bit-identical rows has ONE value
    dv = 2 * gamma(D + 1) * S if kernel == "16" else split_product_bound(S, D)
    E = (dv + EPS * (np.abs(l) + dv))[:, dup_of]
    rows = np.arange(c["M"])
    arg = dup_of[np.argmax(l, -1)]
    lmax = l[rows, arg]
    first = np.where(dup_of[None, :] == arg[:, None], -np.inf, l)   # the best entry outside the winner's group
    second = np.argmax(first, -1) if c["V"] > 1 else arg
    gap = lmax - first[rows, second] if c["V"] > 1 else np.full(c["M"], np.inf)
    decided = gap > E[rows, arg] + E[rows, second]
    cand = l >= lmax[:, None] - (E + E[rows, arg][:, None])
    e_top = np.where(cand, E, 0.0).max(-1)
    d = l - lmax[:, None]
    ex = np.exp(d)
    s = ex.sum(-1)
    p = ex / s[:, None]
    spread = (p * np.abs(d)).sum(-1)
    n = 16 + 2 * vtw_of(kernel, c["V"]) + 3 + 3 * (WAVES[kernel] - 1)
    res = dict(l=l, E=E, arg=arg, decided=decided, cand=cand, lmax=lmax, maxlp=-np.log(s), logs=np.log(s), e_top=e_top,
               mean_e=(p * E).sum(-1), sum_term=gamma(n) + EPS * spread + EPS * np.log(s), unit=EPS * (1 + spread + np.log(s)),
               dup_of=dup_of)
    if c["M"] * c["V"] <= 1 << 21:
        _MODEL[key] = res
    return res


def gather_model(c, layout, res, tgt):
    """float64 tgt_lp per row and its derived bound, from the targets as stored ([B * ld] behind the guard)."""
    M, V = c["M"], c["V"]
    rows = np.arange(M)
    t = tgt[GUARD:][tgt_index(c, rows)].astype(np.int64)
    inside = (t >= 0) & (t < V)
    ts = np.where(inside, t, 0)
    ref = np.where(inside, res["l"][rows, ts] - res["lmax"] - res["logs"], -np.inf)
    derived = res["E"][rows, ts] + res["mean_e"] + res["sum_term"] + EPS * (np.abs(res["l"][rows, ts] - res["lmax"]) + np.abs(np.where(inside, ref, 0.0)))
    return ref, derived, inside


# ================================================================================================ the kernel's scheme in numpy
def emulate_launch(c, layout, kind, bufs, mistakes=()):
    """What a launch leaves in the buffers (a copy), from the kernel's scheme: the fragment map, each wave's walk over its tiles,
    the fold with ties to the lower index and the rescale of the running sum, the half merge, the wave merge, the clamp of rows past
    the count and the targets' row map.  The product itself is float64 rounded once to fp32 (the bound covers the MFMA's order)."""
    bad = set(mistakes)
    assert bad <= set(MISTAKES), bad
    f32 = np.float32
    kernel = LAYOUTS[layout][3]
    M, V = c["M"], c["V"]
    waves, vtw = WAVES[kernel], vtw_of(kernel, V)
    P = 32 * waves * vtw
    out = copy_of(bufs)
    o = operands(c, layout, bufs, w_layout="bf16" if "half_pack_as_bf16" in bad else None)
    (hh, hl), (Wh, Wl) = o["h"], o["W"]
    prod = hh @ Wh.T
    if kernel == "split":
        if "split_no_wlo_xhi" not in bad:
            prod = prod + hh @ Wl.T
        if "split_no_whi_xlo" not in bad:
            prod = prod + hl @ Wh.T
    acc = np.zeros((M, P), f32)
    acc[:, :V] = prod.astype(f32)
    bias = np.full(P, 0.0 if "pad_bias_zero" in bad else -np.inf, f32)
    bias[:V] = 0.0 if "no_bias" in bad else bufs["b"]
    L = (acc + bias[None]).reshape(M, waves, vtw, 32)
    count = live_count(c)
    gather, lse = kind == "gather", kind != "argmax"
    tg = np.full(M, -1, np.int64)
    if gather and count > 0:
        src = np.minimum(np.arange(M), count - 1)  # a lane past the count takes the last live row's target (and is not stored)
        tg = bufs["tgt"][GUARD:][tgt_index(c, src, "gather_ld_as_u" in bad)].astype(np.int64)
    r = np.arange(16)
    entry = (r & 3) + 8 * (r >> 2)
    stats = {}
    with np.errstate(all="ignore"):
        for w in range(waves):
            for hf in range(2):
                m_run, s_run, i_run = np.full(M, NEG_FILL, f32), np.zeros(M, f32), np.zeros(M, np.int64)
                tv = np.full(M, -np.inf, f32)
                for t in range(vtw - 1 if "last_tile_dropped" in bad else vtw):
                    vbase = 32 * (w * vtw + t) + (0 if "half_offset_dropped" in bad else 4 * hf)
                    idx = vbase + (r if "map_r" in bad else entry)
                    vals = L[:, w, t, 4 * hf + entry]                       # accumulator element r holds this entry, whatever it is called
                    tmax, tidx = np.full(M, -np.inf, f32), np.zeros(M, np.int64)
                    for e in range(16):
                        v = vals[:, e]
                        up = v >= tmax if "tie_high_fold" in bad else v > tmax
                        tmax, tidx = np.where(up, v, tmax), np.where(up, idx[e], tidx)
                        if gather:
                            tv = np.where(idx[e] == tg, v, tv)
                    tie = tidx > i_run if "tie_high_fold" in bad else tidx < i_run
                    up = (tmax > m_run) | ((tmax == m_run) & tie)
                    if lse and "no_rescale" not in bad:
                        s_run = np.where(up, s_run * np.exp(m_run - tmax), s_run).astype(f32)
                    m_run, i_run = np.where(up, tmax, m_run), np.where(up, tidx, i_run)
                    if lse:
                        ps = np.zeros(M, f32)
                        for e in range(16):
                            ps = ps + np.exp(vals[:, e] - m_run)
                        s_run = s_run + ps
                stats[(w, hf)] = (m_run, s_run, i_run, tv)

        def merge(a, b_, high, rescale=True):
            (am, as_, ai, at), (om, os_, oi, ot) = a, b_
            nm = np.maximum(am, om)
            s = (as_ * np.exp(am - nm) + os_ * np.exp(om - nm)).astype(f32) if rescale else as_ + os_
            take = (om > am) | ((om == am) & ((oi > ai) if high else (oi < ai)))
            return nm, s, np.where(take, oi, ai), np.maximum(at, ot)

        per_wave = [merge(stats[(w, 0)], stats[(w, 1)], "tie_high_half" in bad) for w in range(waves)]
        best = per_wave[0]
        for w in range(1, waves):
            best = merge(best, per_wave[w], "tie_high_wave" in bad, "wave_merge_no_rescale" not in bad)
        bm, bs, bi, bt = best
        logs = np.log(bs).astype(f32)
        rows = np.arange(M if "m_dev_ignored" in bad else min(count, M))
        if gather:
            val = bt if "gather_returns_logit" in bad else ((bt - bm).astype(f32) - logs).astype(f32)
            out["tgt_lp"][GUARD + tgt_index(c, rows, "gather_ld_as_u" in bad)] = val[rows]
        else:
            out["arg"][GUARD + rows] = bi[rows]
            if kind == "lse":
                out["maxlp"][GUARD + rows] = (bm if "maxlp_is_max_logit" in bad else -logs)[rows]
    return out


# ================================================================================================ the checks
class LaunchError(AssertionError):
    """A launch that fails check_launch.  check: "untouched", "argmax-range", "argmax-decided", "argmax-candidate", "argmax-tie",
    "maxlp-bound", "tgt-inf" or "tgt-bound"; ratio: the worst |err| / bound of a bound failure."""

    def __init__(self, check, text, ratio=None):
        super().__init__(f"[{check}] {text}")
        self.check, self.ratio = check, ratio


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check_launch(c, layout, kind, before, after, worst=None, enforce=True):
    """The checks of the module's docstring.  ``worst`` receives maxlp / tgt (worst |err| / bound), fast (worst (|err| - derived) /
    unit: what FAST is measured from) and undecided (the fraction of undecided rows).  enforce=False: the bounds are measured, not
    asserted (everything else still raises)."""
    who = f"{layout} {c['name']} {kind}"
    kernel = LAYOUTS[layout][3]
    M, V = c["M"], c["V"]
    count = min(live_count(c), M)
    rows = np.arange(count)
    live = {"arg": GUARD + rows, "maxlp": GUARD + rows, "tgt_lp": GUARD + tgt_index(c, rows)}
    for name, b in before.items():
        if b is None:
            continue
        same = _bits(b) == _bits(after[name])
        if name in live:
            same[live[name]] = True
        if not same.all():
            at = int(np.flatnonzero(~same)[0])
            raise LaunchError("untouched", f"{who}: {name}[{at - GUARD}] was written and is not the launch's to write ({int((~same).sum())} such elements)")
    res = model_of(c, layout, before)
    stat = dict(maxlp=0.0, tgt=0.0, fast=-math.inf, undecided=0.0)

    def bound_check(check, got, ref, derived):
        got, ref, derived = got[:count].astype(np.float64), ref[:count], derived[:count]
        err = np.abs(got - ref)
        err = np.where(np.isnan(err), np.inf, err)
        bound = np.minimum(derived + FAST * res["unit"][:count], CAP[kernel])
        ratio = float((err / bound).max()) if count else 0.0
        if count:
            stat["fast"] = max(stat["fast"], float(((err - derived) / res["unit"][:count]).max()))
        if enforce and ratio > 1.0:
            at = int(np.argmax(err / bound))
            raise LaunchError(check, f"{who}: |err| {err[at]:.3e} > bound {bound[at]:.3e} at row {at}: got {got[at]:.7g}, fp64 {ref[at]:.7g}; "
                              f"{int((err > bound).sum())} rows out of bound", ratio)
        return ratio

    if kind == "gather":
        ref, derived, inside = gather_model(c, layout, res, before["tgt"])
        got = after["tgt_lp"][live["tgt_lp"]]
        out = ~inside[:count]
        if not (np.isneginf(got[out])).all():
            at = int(np.flatnonzero(out & ~np.isneginf(got))[0])
            raise LaunchError("tgt-inf", f"{who}: row {at}'s target lies outside [0, {V}) and its result is {got[at]}, not -inf")
        fin = np.where(out, 0.0, got)
        stat["tgt"] = bound_check("tgt-bound", fin, np.where(inside, ref, 0.0), derived)
    else:
        got = after["arg"][live["arg"]].astype(np.int64)
        if not ((got >= 0) & (got < V)).all():
            at = int(np.flatnonzero((got < 0) | (got >= V))[0])
            raise LaunchError("argmax-range", f"{who}: arg[{at}] = {got[at]} is no vocabulary entry")
        dec = res["decided"][:count]
        stat["undecided"] = float((~dec).mean()) if count else 0.0
        group = res["dup_of"][got]
        wrong = dec & (group != res["arg"][:count])
        if wrong.any():
            at = int(np.flatnonzero(wrong)[0])
            raise LaunchError("argmax-decided", f"{who}: arg[{at}] = {got[at]}, fp64 {res['arg'][at]} (a decided row); {int(wrong.sum())} such rows")
        notcand = ~dec & ~res["cand"][rows, got]
        if notcand.any():
            at = int(np.flatnonzero(notcand)[0])
            raise LaunchError("argmax-candidate", f"{who}: arg[{at}] = {got[at]} is not within its bound of the maximum (fp64 {res['arg'][at]})")
        if (group != got).any():
            at = int(np.flatnonzero(group != got)[0])
            raise LaunchError("argmax-tie", f"{who}: arg[{at}] = {got[at]}: bit-identical entry {group[at]} is lower")
        if kind == "lse":
            stat["maxlp"] = bound_check("maxlp-bound", after["maxlp"][live["maxlp"]], res["maxlp"], res["e_top"] + res["mean_e"] + res["sum_term"])
    if worst is not None:
        worst.update(stat)
