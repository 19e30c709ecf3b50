"""The subsampling front end (csrc/conv1.hip, conv2.hip, gemm.hip) in every launch form of the engine, in both libraries (bf16 and
fp16 operands) where the form exists in both, against the float64 models of frontend_model.py.  Every launch goes through
cn_op_frontend_desc, which selects each kernel by name and reaches what the cn_op_conv* entries cannot: the per-utterance records
of a merged pass (expanded on the device by launch_expand_meta), halo modes 1 and 2, the conv1 -> conv2 hand-off through the
caller's image.  The cases are frontend_model.CASES, one group per call site (the case id names it); test_frontend_model.py shows
on the CPU what the checks catch.

Per launch (frontend_model.run_case): |out - fp64| <= bound on every live element; the RMS of (out - fp64) within RATIO of the
emulation's; border cells and rows past an utterance's own batch bit-zero, the border untouched under halo mode 2, expand_meta's
records and the returned scale bytes equal to the model's; NaN in every frame past an utterance's own, in spare lda columns, in
rows past M and around every input; NaN bytes in every image cell before a halo 0 / 1 launch; a sentinel behind the last output
row and around every output.

Run with -s to see the worst ratios per library, form and output (the table of docs/KERNEL_NOTES.md)."""
import ctypes as C

import numpy as np
import pytest
import torch

import frontend_model as fm
from attention_model import LAYOUTS
from cassnat_asr_public_amd import abi, hip

pytestmark = pytest.mark.gpu

K = abi.CONSTANTS
WORST = {}
CONV1 = {"plain": "PLAIN", "planes": "PLANES", "mix": "MIXPLANES", "f8v": "F8_VALU", "f8m": "F8_MFMA", "m16": "BF16_MFMA"}
CONV2 = {"generic": "GENERIC", "dma": "DMA", "x3": "X3", "mix": "MIX", "f8": "F8"}
LINEAR = {"generic": "GENERIC", "dma": "DMA", "f8": "F8"}
PREC = {"16": "bf16", "f32": "fp32", "x3": "bf16x3"}


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    print("\nworst |out - fp64| / bound and rms(out - fp64) / yardstick per library, form, format and output:")
    for (layout, form, fmt, name), (b, r) in sorted(WORST.items()):
        print(f"  {layout:5s} {form:34s} {fmt:6s} {name:6s} {b:.3f}  {r:.3f}")
    for layout in fm.LIBS:
        rs = [v for k, v in WORST.items() if k[0] == layout]
        if rs:
            print(f"  {layout}: worst bound ratio {max(b for b, _ in rs):.3f}, worst rms ratio {max(r for _, r in rs):.3f}")
    fm._MODEL.clear()
    fm._W.clear()


def dev(whole):
    return torch.from_numpy(whole).cuda()


def ptr(t, off=fm.GUARD):
    return None if t is None else t.data_ptr() + off


def launch(call):
    """One cn_op_frontend_desc call on copies of the call's host buffers; returns them afterwards (host)."""
    c, layout, st = call["c"], call["layout"], call["stages"]
    flavour, _, operand = LAYOUTS[layout]
    L = hip.lib(flavour)
    assert L.cn_operand16().decode() == operand
    prec = LAYOUTS["fp16" if layout == "fp16" else PREC[c.get("prec", "16")]][1]
    f = dict(precision=prec, halo=call["halo"])
    keep = []
    q8 = (C.c_int32 * 8)()
    f["q8_out"] = C.addressof(q8)
    if c["kind"] != "linear":
        f.update(B=c["B"], T=c["T"], F=c["F"], C=c["C"])
        img = dev(call["img"])
        f["img"] = ptr(img)
    meta = None
    if "conv1" in st:
        cc = c if c["kind"] == "conv1" else fm.conv1_of(c)
        s1, s2 = fm.scales_of(cc)
        xw, xi = fm.guarded(call["x"].numel() * 4, 0xff)
        xi[:] = call["x"].contiguous().numpy().view(np.uint8).reshape(-1)
        w9c, b1 = fm.weights1(c["C"])
        keep += [dev(xw), w9c.cuda(), b1.cuda()]
        f.update(conv1_form=K["CN_FE_CONV1_" + CONV1[cc["form"]]], x=ptr(keep[-3]), w9c=ptr(keep[-2], 0), bias1=ptr(keep[-1], 0), img_scale=s1,
                 img_scale2=s2)
        if call["subs"]:
            n = len(call["subs"])
            rows, frames = (C.c_int32 * n)(*[r for r, _ in call["subs"]]), (C.c_int32 * n)(*[t for _, t in call["subs"]])
            meta = torch.full((c["B"], 4), -1, dtype=torch.int32).cuda()
            keep += [rows, frames]
            f.update(n_sub=n, sub_rows=C.addressof(rows), sub_frames=C.addressof(frames), meta_out=ptr(meta, 0))
    if "conv2" in st:
        w2, b2 = fm.weights2(c["C"])
        out = dev(call["out"])
        keep += [w2, b2.cuda()]
        f.update(conv2_form=K["CN_FE_CONV2_" + CONV2[c["form"]]], w2=w2.data_ptr(), bias2=ptr(keep[-1], 0), c2_out=ptr(out), out8_scale=c["out8"])
        if c["form"] == "f8":
            f["img_scale"] = c["scale"]
    if "linear" in st:
        w, b = fm.weights_lin(c["K"])
        a, out = dev(call["a"]), dev(call["out"])
        pe = None if call["pe"] is None else call["pe"].cuda()
        keep += [w, b.cuda(), a, pe]
        f.update(linear_form=K["CN_FE_LINEAR_" + LINEAR[c["form"]]], lin_a=ptr(a), lin_w=w.data_ptr(), lin_bias=ptr(keep[-3], 0), lin_out=ptr(out),
                 M=c["M"], K=c["K"], lda=c["lda"], a_scale=c["a_scale"], scale=fm.LIN_SCALE, pe=ptr(pe, 0), pe_period=c["period"])
    d = hip.CnFrontendDesc(**f)
    hip.check(L.cn_op_frontend_desc(C.byref(d), hip.current_stream()), "cn_op_frontend_desc", L)
    torch.cuda.synchronize()
    res = {"q8": list(q8), "meta": None if meta is None else meta.cpu().numpy()}
    if c["kind"] != "linear":
        res["img"] = img.cpu().numpy()
    if "conv2" in st or "linear" in st:
        res["out"] = out.cpu().numpy()
    return res


CASES = [(c, layout) for c in fm.CASES for layout in c["libs"]]


@pytest.mark.parametrize("c,layout", CASES, ids=[f"{c['name']}@{c['site']}@{layout}".replace(" ", "_") for c, layout in CASES])
def test_launch_against_float64(c, layout):
    seen = {}
    try:
        fm.run_case(c, layout, launch, seen)
    finally:
        for (_, form, fmt, name), (b, r) in seen.items():
            print(f"{layout} {c['name']} {form} {fmt} {name}: |err| / bound {b:.3f}, rms / yardstick {r:.3f}")
            old = WORST.get((layout, form, fmt, name), (0.0, 0.0))
            WORST[(layout, form, fmt, name)] = (max(old[0], b), max(old[1], r))
