"""The tiled GEMM (csrc/gemm.hip) in every instantiation and launch form of the engine, in both libraries, against the float64
model of gemm_model.py.  Every launch goes through cn_op_gemm_desc, which reaches all of GemmArgs' non-convolution product; the
cases are gemm_model.CASES, one group per call site (the case id names it), and test_gemm_model.py shows on the CPU what the
checks catch.  cn_gemm_form must name the instantiation each case is written for before it is launched (test_gemm_args.py shows
that the cases reach every one).

Per launch (gemm_model.check_launch): |out - fp64| <= bound on every live element (a split-bf16 output: both halves); the RMS of
(out - fp64) within RATIO of the yardstick; every input and every element of C the launch does not own bit for bit as before -
NaN in A's rows past M and columns K .. lda, resid's columns N .. ldr, pe's rows past the period and around every input, a
sentinel in C's columns N .. ldc, rows past M and around it.

Run with -s to see the worst ratios per library, form, epilogue and output (the table of docs/KERNEL_NOTES.md)."""
import ctypes as C

import pytest
import torch

import gemm_model as gm
from cassnat_asr_public_amd import hip

pytestmark = pytest.mark.gpu

WORST = {}
EPI_NAMES = ((gm.RELU, "relu"), (gm.SWISH, "swish"), (gm.EMBED, "embed"), (gm.RESID, "resid"))


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    print("\nworst |out - fp64| / bound, rms(out - fp64) / yardstick and (e4m3 operands) accumulation error / sum |a| |w| deq per "
          "library, form, epilogue and output:")
    for key, (b, r, a) in sorted(WORST.items()):
        print("  %-5s %-6s %-6s %-12s %-5s %.3f  %.3f  %s" % (key + (b, r, "" if a is None else f"{a:.3e}")))
    for layout in gm.LAYOUTS:
        rs = [v for k, v in WORST.items() if k[1] == layout]
        if rs:
            acc = [a for _, _, a in rs if a is not None]
            print(f"  {layout}: worst bound ratio {max(b for b, _, _ in rs):.3f}, worst rms ratio {max(r for _, r, _ in rs):.3f}"
                  + (f", worst accumulation measure {max(acc):.3e}" if acc else ""))
    gm._MODEL.clear()


def lib_of(layout):
    flavour, _, operand = gm.LAYOUTS[layout]
    L = hip.lib(flavour)
    assert L.cn_operand16().decode() == operand
    return L


def launch(c, layout, host):
    """One cn_op_gemm_desc call on copies of the case's host buffers; returns them afterwards (host).  -> (rc, buffers)"""
    L = lib_of(layout)
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in host.items()}
    kinds = dict(A=gm.STORE[layout], W=gm.STORE[layout], C=gm.geometry(c, layout)["okind"])
    address = lambda name: dev[name].data_ptr() + gm.offset_bytes(dev[name], kinds.get(name, "f32"))
    d = gm.descriptor(c, layout, address, host["acc_scale"])
    assert L.cn_gemm_form(C.byref(d)) == gm.form_code(c, layout), (L.cn_gemm_form(C.byref(d)), L.cn_last_error())
    hip.check(L.cn_op_gemm_desc(C.byref(d), hip.current_stream()), "cn_op_gemm_desc", L)
    torch.cuda.synchronize()
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in dev.items()}


@pytest.mark.parametrize("c, layout", gm.PAIRS, ids=[gm.pair_id(c, layout) for c, layout in gm.PAIRS])
def test_launch_against_float64(c, layout):
    before = gm.buffers(c, layout)
    after = launch(c, layout, before)
    seen = {}
    try:
        gm.check_launch(c, layout, before, after, seen)
    finally:
        if seen:
            print(f"{layout} {c['name']}: |err| / bound {seen['bound']:.3f}, rms / yardstick {seen['rms']:.3f}"
                  + (f", accumulation / sum |a||w| {seen['acc']:.3e}" if "acc" in seen else ""))
            epi = "+".join(n for bit, n in EPI_NAMES if c["epi"] & bit) or "none"
            key = (gm.LAYOUTS[layout][2], layout, c["tile"], epi, c["out"])
            old = WORST.get(key, (0.0, 0.0, None))
            acc = seen.get("acc")
            WORST[key] = (max(old[0], seen["bound"]), max(old[1], seen["rms"]), acc if old[2] is None else max(old[2], acc or 0.0))


@pytest.mark.parametrize("layout", list(gm.LAYOUTS))
def test_nothing_to_launch_leaves_every_sentinel(layout):
    """M = 0 and N = 0: rc 0 and C untouched."""
    c = next(c for c in gm.CASES if c["name"] == ("f8-qkv-k128" if layout == "e4m3" else "shape-M63-N33-s2"))
    L = lib_of(layout)
    host = gm.buffers(c, layout)
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in host.items()}
    kinds = dict(A=gm.STORE[layout], W=gm.STORE[layout], C=gm.geometry(c, layout)["okind"])
    address = lambda name: dev[name].data_ptr() + gm.offset_bytes(dev[name], kinds.get(name, "f32"))
    for field in ("M", "N"):
        d = gm.descriptor(c, layout, address, host["acc_scale"])
        setattr(d, field, 0)
        assert L.cn_gemm_form(C.byref(d)) >> 8 == gm.TILE["none"]
        assert L.cn_op_gemm_desc(C.byref(d), hip.current_stream()) == 0
    torch.cuda.synchronize()
    for name, t in host.items():
        if torch.is_tensor(t):
            assert torch.equal(gm.bits(dev[name].cpu()), gm.bits(t)), name
