"""The fused feed-forward sublayer (csrc/fused.hip: ffn_fused_kernel, and its d_ff-split form finished by ffn_reduce_kernel) as
cn_op_ffn_fused_act launches it: the buffers, the cases and the checks.  Shared by the kernel test (test_gpu_ffn.py) and the CPU
test that shows what the checks catch (test_ffn_model.py).

The operation is chain_model.chain_model(x, ctx=None, ..., tail_n=0) with the next LayerNorm on or off:

    x += W2 . act(W1 . LN1(x) + b1) + b2;   xn_out = LNn(x) in the library's 16-bit type, where nln is given

and the float64 model, its bound and its emulation are chain_model's.  What this module adds is the split form's own arithmetic:
nslice fp32 partial sums added in slice order, then (x + acc) + b2 - gamma(nslice + 2) on the magnitudes involved, in the bound of
x (carried through LNn) and, as a random-walk term, in the yardstick.

The buffers: x (float32) and xn_out (16-bit) of M rows between GUARD_ROWS rows of a sentinel that must come back bit for bit;
xn_out's live rows hold NaN before the launch and must be finite after it (untouched, like everything else, without a next
LayerNorm).  The partial sums live in the entry's own scratch and cannot be guarded from here."""
import torch

import chain_model as cm
from attention_model import EPS, gamma, out_ulp

D = cm.D
GUARD_ROWS = 8
SENTINEL = cm.SENTINEL
LIBS = cm.LIBS

# what the aggregate check allows, RMS(result - fp64) / yardstick: chain_model.RATIO to start with (the same arithmetic in another
# kernel), re-measured on the MI355X over every case of CASES (docs/KERNEL_NOTES.md, "Generic GEMM and fused feed-forward: float64
# tests of every launch form"): at most 1.0057 (bf16) and 1.0145 (fp16), both on LNn(x) of swish-dff1024-s4-next-M35-adversarial.
# fp16 keeps chain_model's 1.25 (a factor 1.23 above the measurement, 5.2 below the smallest mistake, the biased std at 6.57);
# bf16 takes 1.21 for the factor 1.2 (chain_model's 1.1 leaves 1.09) - below every mistake test_ffn_model.py requires it to catch
# (7.4 at the least), and below the two 0.2 % LayerNorm mistakes it only reports (1.24, 1.36).
RATIO = dict(cm.RATIO, bf16=1.21)
assert RATIO["fp16"] == 1.25

MISTAKES = ("ln1_biased_std", "lnn_biased_std", "ln1_eps_in_var", "lnn_eps_in_var", "no_b1", "no_b2", "no_residual_ffn", "act_swapped",
            "slice_dropped", "slice_twice", "slice_shifted", "lnn_from_old_x", "rows_past_m_stored")
CHAIN_MISTAKES = MISTAKES[:8]  # chain_model's own: they change its emulation


def case(name, site, M, dff, nslice=1, swish=False, has_next=True, adv=False, tiny_w2=False):
    """tiny_w2: W2 and b2 scaled by 2^-20, so that the adversarial rows (a nearly constant one among them) reach the NEXT LayerNorm
    nearly unchanged - where eps sits in that norm shows on no other row."""
    assert dff % (128 * nslice) == 0
    c = cm.case(name, site, M, dff=dff, has_next=has_next, swish=swish, adv=adv, ln_to="out" if has_next else None)
    c["nslice"], c["tiny_w2"] = nslice, tiny_w2
    return c


_W = {}


def weights_of(c):
    """chain_model's weights of the (d_ff, 0) form; tiny_w2: a copy with W2 and b2 scaled down."""
    w = cm.weights_of(c)
    if not c["tiny_w2"]:
        return w
    if c["dff"] not in _W:
        _W[c["dff"]] = dict(w, w2=(w["w2"] * 2.0 ** -20).contiguous(), b2=(w["b2"] * 2.0 ** -20).contiguous())
    return _W[c["dff"]]


M_ALL = (1, 31, 32, 33, 63, 64, 65, 129)  # <= 32: the MT = 1 kernel, above: MT = 2


def _cases():
    out = []

    def add(site, M, dff, nslice, swish, has_next, adv=False, tiny_w2=False):
        name = (f"{'swish' if swish else 'relu'}-dff{dff}-s{nslice}-{'next' if has_next else 'last'}-M{M}" + ("-adversarial" if adv else "")
                + ("-tinyw2" if tiny_w2 else ""))
        out.append(case(name, site, M, dff, nslice, swish, has_next, adv, tiny_w2))

    # ---- the whole sublayer in one launch: every M with both activations, with and without the next LayerNorm, d_ff by turns
    dffs = (128, 256, 1024, 2048)
    for i, M in enumerate(M_ALL):
        for swish in (False, True):
            for has_next in (True, False):
                add("run_ffn", M, dffs[(i + swish + 2 * has_next) % 4], 1, swish, has_next)
    # ---- the two launches of decode_ar.hip: run_ffn_step (a few rows, d_ff split, next LayerNorm), both activations
    for M in (1, 32, 33):
        for swish in (False, True):
            add("decode_ar.hip run_ffn_step 2048 / 8", M, 2048, 8, swish, True)
            add("decode_ar.hip run_ffn_step 512 k / 4", M, 1024, 4, swish, True)
    add("decode_ar.hip run_ffn_step 512 k / 4", 33, 2048, 4, True, True)
    # ---- every slice count that divides, with and without the next LayerNorm
    for i, (dff, ns) in enumerate(((256, 2), (1024, 2), (1024, 8), (2048, 2), (2048, 16))):
        add("d_ff split", (65, 1, 129, 31, 64)[i], dff, ns, bool(i % 2), bool(i % 2))
        add("d_ff split", (1, 65, 32, 129, 33)[i], dff, ns, not i % 2, not i % 2)
    # ---- rows that stress the LayerNorms (chain_model.inputs: a nearly constant last row, one channel at 1e3 in row 31, a row of zeros at 32)
    add("run_ffn", 129, 2048, 1, False, True, adv=True)
    add("run_ffn", 129, 1024, 1, True, True, adv=True)
    add("decode_ar.hip run_ffn_step 512 k / 4", 35, 1024, 4, True, True, adv=True)
    add("decode_ar.hip run_ffn_step 2048 / 8", 35, 2048, 8, False, True, adv=True)
    # ... and the same rows in front of the next LayerNorm
    add("run_ffn", 35, 256, 1, False, True, adv=True, tiny_w2=True)
    add("decode_ar.hip run_ffn_step 512 k / 4", 35, 1024, 4, True, True, adv=True, tiny_w2=True)
    return out


CASES = _cases()


def case_id(c):
    return f"{c['name']}@{c['site']}".replace(" ", "_")


def buffers(c, layout):
    """x (float32) and xn (the layout's 16-bit type), flat, M rows of 256 between GUARD_ROWS sentinel rows; xn's live rows NaN."""
    x, _ = cm.inputs(c, layout)
    M, G = c["M"], GUARD_ROWS
    xb = torch.full(((M + 2 * G) * D,), SENTINEL)
    xb[G * D:(G + M) * D] = x.reshape(-1)
    nb = torch.full(((M + 2 * G) * D,), SENTINEL, dtype=cm.DTYPES[layout])
    nb[G * D:(G + M) * D] = cm.NAN
    return dict(x=xb, xn=nb)


def live(buf, M):
    return buf[GUARD_ROWS * D:(GUARD_ROWS + M) * D].view(M, D)


def hidden_emulation(x, w, layout, swish, eps=1e-6):
    """The hidden activations as the kernel holds them (rounded to the operand), float64 (M, d_ff): what a slice's partial sum is
    made of - chain_model's emulation of the first half, here only to take slices of it (the slice mistakes)."""
    dt = cm.DTYPES[layout]
    rop = lambda t: t.float().to(dt).double()
    y, _ = cm.layer_norm64(x.double(), torch.zeros_like(x.double()), w["a1"].double(), w["b1n"].double(), eps)
    pre = rop(y) @ w["w1"].to(dt).double().T + w["b1"].double()
    return rop(pre * torch.sigmoid(pre) if swish else torch.relu(pre))


_MODEL = {}


def model_of(c, layout):
    """chain_model of the case with the split form's terms added -> dict(x, ln: (fp64, bound, emulation, accumulation rms term))."""
    key = (c["name"], layout)
    if key in _MODEL:
        return _MODEL[key]
    x, _ = cm.inputs(c, layout)
    w = weights_of(c)
    res = cm.chain_model(x, None, w, layout, c["dff"], 0, c["has_next"], c["swish"])
    X, dX, E, acc = res["x"]
    ns = c["nslice"]
    if ns > 1:
        h = hidden_emulation(x, w, layout, c["swish"])
        mag = h.abs() @ w["w2"].to(cm.DTYPES[layout]).double().abs().T + w["b2"].double().abs() + x.double().abs()
        dX = dX + gamma(ns + 2) * mag
        acc = (acc ** 2 + (EPS * X.abs()) ** 2 * (ns + 2)).sqrt()
    out = {"x": (X, dX, E, acc), "ln": None}
    if c["has_next"]:
        y, dy = cm.layer_norm64(X, dX, w["na"].double(), w["nb"].double(), 1e-6)
        half = 0.5 * torch.maximum(out_ulp(y.abs() + dy, layout), torch.full_like(y, 2 * cm.U_SUB[layout]))
        out["ln"] = (y, dy + half, res["ln"][2], res["ln"][3])
    _MODEL[key] = out
    return out


def emulate_launch(c, layout, b, mistakes=()):
    """What a launch leaves in the buffers ``b`` (in place), from the emulation: a stand-in for the kernel on the CPU."""
    bad = set(mistakes)
    assert bad <= set(MISTAKES), bad
    M, w = c["M"], weights_of(c)
    x = live(b["x"], M).clone()
    res = cm.chain_model(x, None, w, layout, c["dff"], 0, c["has_next"], c["swish"], mistakes=bad & set(CHAIN_MISTAKES))
    E = res["x"][2]
    ln = res["ln"][2] if c["has_next"] else None
    slices = bad & {"slice_dropped", "slice_twice", "slice_shifted"}
    if slices:
        h = hidden_emulation(x, w, layout, c["swish"])
        W2 = w["w2"].to(cm.DTYPES[layout]).double()
        width = c["dff"] // c["nslice"]
        s = c["nslice"] // 2
        part = lambda lo: h[:, lo:lo + width] @ W2[:, lo:lo + width].T
        if "slice_dropped" in bad:
            E = E - part(s * width)
        if "slice_twice" in bad:
            E = E + part(s * width)
        if "slice_shifted" in bad:  # the slice takes its hidden units one 32-unit tile further on (wrapping at d_ff)
            lo = s * width
            E = E - h[:, lo:lo + 32] @ W2[:, lo:lo + 32].T
            nx = (lo + width) % c["dff"]
            E = E + h[:, nx:nx + 32] @ W2[:, nx:nx + 32].T
        E = E.float().double()
    if c["has_next"] and (slices or "lnn_from_old_x" in bad):
        src = x.double() if "lnn_from_old_x" in bad else E
        y, _ = cm.layer_norm64(src, torch.zeros_like(src), w["na"].double(), w["nb"].double(), 1e-6)
        ln = y.float().to(cm.DTYPES[layout]).double()
    rows = M + 1 if "rows_past_m_stored" in bad else M
    if rows > M:
        E = torch.cat([E, E[-1:]], 0)
        ln = None if ln is None else torch.cat([ln, ln[-1:]], 0)
    live(b["x"], rows)[:] = E.float()
    if ln is not None:
        live(b["xn"], rows)[:] = ln.to(b["xn"].dtype)
    return b


LaunchError = cm.LaunchError


def check_launch(c, layout, before, after, worst=None, enforce=True):
    """chain_model.check_launch's checks on x and xn_out: the guards (and the whole of xn_out without a next LayerNorm) bit for bit
    as before, every live element of xn_out finite, |out - fp64| <= bound on every live element, the RMS of (out - fp64) within
    RATIO of the yardstick.  ``worst``: receives {output: (bound ratio, rms ratio)}; enforce=False: measure only."""
    M, G = c["M"], GUARD_ROWS
    res = model_of(c, layout)
    for name in ("x", "xn"):
        same = cm.bits(before[name]) == cm.bits(after[name])
        if name == "x" or c["has_next"]:
            same[G * D:(G + M) * D] = True
        if not bool(same.all()):
            where = int((~same).nonzero()[0])
            raise LaunchError("untouched", f"{layout} {c['name']}: {name}[{where}] (row {where // D - G}) was written and is not the "
                              f"launch's to write ({int((~same).sum())} such elements)")
    outs = [("x", "x")] + ([("ln", "xn")] if c["has_next"] else [])
    rms = lambda t: float(t.pow(2).mean().sqrt())
    for name, buf in outs:
        ref, bound, emu, acc = res[name]
        got = live(after[buf], M).double()
        if not bool(torch.isfinite(got).all()):
            raise LaunchError("bound", f"{layout} {c['name']} {name}: {int((~torch.isfinite(got)).sum())} live elements are not finite")
        err = (got - ref).abs()
        if enforce and not bool((err <= bound).all()):
            badm = ~(err <= bound)
            at = tuple(int(v) for v in badm.nonzero()[0])
            raise LaunchError("bound", f"{layout} {c['name']} {name}: |err| {float(err[at]):.3e} > bound {float(bound[at]):.3e} at "
                              f"(row, column) = {at}; got {float(got[at]):.6g}, fp64 {float(ref[at]):.6g}; {int(badm.sum())} elements "
                              "out of bound")
        yard = (rms(emu - ref) ** 2 + rms(acc) ** 2) ** 0.5
        ratio = rms(got - ref) / yard if yard > 0 else (0.0 if rms(got - ref) == 0 else float("inf"))
        if worst is not None:
            worst[name] = (float((err / bound.clamp(min=1e-300)).max()), ratio)
        if enforce and not ratio <= RATIO[layout]:
            raise LaunchError("ratio", f"{layout} {c['name']} {name}: rms(result - fp64) {rms(got - ref):.3e} is {ratio:.2f} x the "
                              f"yardstick {yard:.3e} (emulation {rms(emu - ref):.3e}); allowed {RATIO[layout]}", ratio)
