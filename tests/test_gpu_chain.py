"""The row-chain kernel (csrc/chain.hip) in every launch form of the engine, in both libraries (bf16 and fp16 operands), against the
float64 model of chain_model.py.  Every launch goes through cn_op_chain_desc, which reaches all of ChainArgs; the cases are
chain_model.CASES, one group per call site (the case id names it), and test_chain_model.py shows on the CPU what the checks catch.

Per launch (chain_model.check_launch): |out - fp64| <= bound on every live element of x, LNn(x) and the tail; the RMS of
(out - fp64) within RATIO of the emulation's; x untouched bit for bit where the launch does not store it; NaN in every spare input
column and dead input row, a sentinel in every spare output column, row and block that must survive (the rows of a blocked
form's last 32-row block past the live ones are the launch's to write: test_gpu_attention_proj.py).

Run with -s to see the worst ratios per library, form and output (the table of docs/KERNEL_NOTES.md)."""
import ctypes as C
import math

import pytest
import torch

import chain_model as cm
from attention_model import LAYOUTS
from cassnat_asr_public_amd import hip

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    print("\nworst |out - fp64| / bound and rms(out - fp64) / yardstick per library, form and output:")
    for (layout, form, name), (b, r) in sorted(WORST.items()):
        print(f"  {layout:5s} {form:20s} {name:5s} {b:.3f}  {r:.3f}")
    for layout in cm.LIBS:
        rs = [v for k, v in WORST.items() if k[0] == layout]
        if rs:
            print(f"  {layout}: worst bound ratio {max(b for b, _ in rs):.3f}, worst rms ratio {max(r for _, r in rs):.3f}")


@pytest.fixture(scope="module")
def shared():
    """Host weights per (d_ff, tail) and the float64 model per case and layout, computed once and left unchanged: the entry packs
    host weights per call, so the cases of a form share their tensors through chain_model's caches, dropped when the module ends."""
    yield cm
    cm._MODEL.clear()
    cm._W.clear()


def lib_of(layout):
    flavour, _, operand = LAYOUTS[layout]
    L = hip.lib(flavour)
    assert L.cn_operand16().decode() == operand
    return L


def hp(t):
    return None if t is None else t.data_ptr()


def launch(c, layout, host, f8=False):
    """Launch case ``c`` on copies of the host buffers; returns the buffers afterwards (host)."""
    L = lib_of(layout)
    w = cm.weights_of(c)
    dev = {k: (None if v is None else v.cuda()) for k, v in host.items()}
    rows = None if c["rows"] is None else torch.tensor([c["rows"]], dtype=torch.int32).cuda()
    has_ctx, has_next = c["ctx"] is not None, c["has_next"]
    d = hip.CnChainDesc(
        x=hp(dev["x"]), ctx=hp(dev["ctx"]), ldctx=c["ldctx"], ctx_blocked=int(c["ctx"] == "blk"),
        wo=hp(w["wo"]) if has_ctx else None, bo=hp(w["bo"]) if has_ctx else None,
        ln1_a=hp(w["a1"]), ln1_b=hp(w["b1n"]), w1=hp(w["w1"]), b1=hp(w["b1"]), w2=hp(w["w2"]), b2=hp(w["b2"]),
        nln_a=hp(w["na"]) if has_next else None, nln_b=hp(w["nb"]) if has_next else None, wt=hp(w["wt"]), bt=hp(w["bt"]),
        out=hp(dev["out"]), ln_out=hp(dev["ln_out"]), ldo=c["ldo"], ld_ln=c["ld_ln"] if dev["ln_out"] is not None else 0,
        M=c["M"], dff=c["dff"], tail_n=c["tail"], eps=1e-6, ln_blocked=int(c["ln_blk"]), out_blocked=int(c["out_blk"]),
        store_x=int(c["store_x"]), x_in_blocked=int(c["xin_blk"]), x_out_blocked=int(c["xout_blk"]), swish=int(c["swish"]),
        f8=int(f8), rows_dev=hp(rows))
    hip.check(L.cn_op_chain_desc(C.byref(d), hip.current_stream()), "cn_op_chain_desc", L)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu()) for k, v in dev.items()}


@pytest.mark.parametrize("layout", cm.LIBS)
@pytest.mark.parametrize("c", cm.CASES, ids=[f"{c['name']}@{c['site']}".replace(" ", "_") for c in cm.CASES])
def test_launch_against_float64(shared, c, layout):
    before = shared.buffers(c, layout)
    after = launch(c, layout, before)
    seen = {}
    try:
        shared.check_launch(c, layout, before, after, seen)
    finally:
        for (_, form, name), (b, r) in seen.items():
            print(f"{layout} {c['name']} {name}: |err| / bound {b:.3f}, rms / yardstick {r:.3f}")
            old = WORST.get((layout, form, name), (0.0, 0.0))
            WORST[(layout, form, name)] = (max(old[0], b), max(old[1], r))


def _e4m3(t):
    return t.clamp(-448, 448).to(torch.float8_e4m3fn).float()


def test_fp8_feed_forward_with_blocked_ctx(shared):
    """x_mode bit 32 through the descriptor, in the form the fp8 engine launches: an fp8 engine with row chains runs the bf16
    engine's encoder path (model.hip), so its chain launches read the attention kernel's blocked ctx, x blocked in and out, a
    blocked Q|K|V tail.  (run_enc_layer_fp8 is the unfused path: it never launches this kernel.)  Emulation and tolerances of
    test_gpu_kernels.py::test_chain_fp8_feed_forward; a per-element bound for e4m3 byte flips is out of scope."""
    import torch.nn.functional as F

    from oracle.cassnat_oracle import layer_norm

    c, layout = cm.F8_CASE, "bf16"
    M = c["M"]
    w = cm.weights_of(c)
    x, ctx = cm.inputs(c, layout)
    r16 = lambda t: t.to(torch.bfloat16).float()
    relerr = lambda a, b: ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()
    ref = x + F.linear(ctx.float(), r16(w["wo"]), w["bo"])
    pow2 = lambda t: 2.0 ** math.floor(math.log2(448.0 / t.abs().max().item()))
    s1, s2 = pow2(w["w1"]), pow2(w["w2"])
    xn8 = _e4m3(layer_norm(ref, w["a1"], w["b1n"]) * 16.0)
    h8 = _e4m3(F.relu(F.linear(xn8, _e4m3(w["w1"] * s1)) / (s1 * 16.0) + w["b1"]) * 8.0)
    ref = ref + F.linear(h8, _e4m3(w["w2"] * s2)) / (s2 * 8.0) + w["b2"]
    before = cm.buffers(c, layout)
    after = launch(c, layout, before, f8=True)
    pl = cm.places(c)
    xo = after["x"][pl["x"][1]]
    print(f"f8 blocked ctx: x relerr {relerr(xo, ref):.2e}")
    assert relerr(xo, ref) < 8e-3
    out = after["out"][pl["tail"][1]]
    want = F.linear(r16(layer_norm(xo, w["na"], w["nb"])), r16(w["wt"]), w["bt"])
    print(f"f8 blocked ctx: tail relerr {relerr(out, want):.2e}")
    assert relerr(out, want) < 6e-3
    # the blocks past the last one that holds rows keep their sentinel
    assert bool((after["out"][cm.rows32(M) * c["ldo"]:] == cm.SENTINEL).all())
    assert bool(torch.isnan(after["x"][cm.rows32(M) * cm.D:]).all())
