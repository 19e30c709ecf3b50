"""The descriptor entry of the tiled GEMM (cn_op_gemm_desc), the host-only query of the form a call takes (cn_gemm_form) and
their argument checks.  No device needed: every call below is refused, or decided, before anything is launched.  The kernel itself
is compared with a float64 model in test_gpu_gemm.py."""
import ctypes as C

import numpy as np
import pytest

import gemm_model as gm
from cassnat_asr_public_amd import abi, hip

K_ = abi.CONSTANTS
FLAVOURS = [None, "f16"]
OWN16 = {None: K_["CN_PRECISION_BF16"], "f16": K_["CN_PRECISION_F16"]}
# a host buffer stands in for every pointer: the calls under test never get as far as reading one
_BUF = np.zeros(1 << 12, np.float32)
P = _BUF.ctypes.data
TILE_OF = {v: k for k, v in gm.TILE.items()}


def desc(flavour=None, **kw):
    """A 16-bit product of the library's own operand type the kernel would accept, with ``kw`` overriding fields."""
    f = dict(precision=OWN16[flavour], c_kind=gm.OUT["own"], A=P, W=P, bias=P, C=P, lda=128, ldc=40, M=10, N=40, K=128, epi=0,
             pe_period=1, resid_scale=1.0, scale=1.0, acc_scale=1.0, c_scale=1.0)
    f.update(kw)
    return hip.CnGemmDesc(**f)


def refused(L, d, *words):
    for fn, name in ((lambda p: L.cn_op_gemm_desc(p, None), "cn_op_gemm_desc"), (L.cn_gemm_form, "cn_gemm_form")):
        rc = fn(C.byref(d) if d is not None else None)
        msg = L.cn_last_error().decode()
        assert rc != 0, (name, msg)
        assert msg.startswith(name + ": "), msg
        for w in words:
            assert w in msg, (w, msg)


def parts(code):
    return code & 15, code >> 4 & 15, code >> 8


def test_entry_points_are_declared_exported_and_sized_like_the_c_struct():
    names = hip.declared_symbols()
    for name in ("cn_op_gemm_desc", "cn_gemm_desc_size", "cn_gemm_form", "cn_op_gemm"):
        assert name in names
        for flavour in FLAVOURS:
            getattr(hip.lib(flavour), name)
    for flavour in FLAVOURS:
        assert hip.lib(flavour).cn_gemm_desc_size() == C.sizeof(hip.CnGemmDesc) == 120
    assert [n for n, _ in hip.CnGemmDesc._fields_] == [
        "precision", "c_kind", "A", "W", "bias", "C", "resid", "pe", "w_inv_scale", "lda", "ldc", "ldr", "M", "N", "K", "epi",
        "pe_period", "resid_scale", "scale", "ab_fp8", "acc_scale", "c_scale", "reserved"]
    assert [K_["CN_GEMM_EPI_" + n] for n in ("RELU", "RESID", "EMBED", "SWISH")] == [1, 2, 4, 8]  # the values of kernels.h


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refuses_what_the_issue_lists(flavour):
    L = hip.lib(flavour)
    d = lambda **kw: desc(flavour, **kw)
    refused(L, None, "null descriptor")
    for name in ("A", "W", "C"):
        refused(L, d(**{name: None}), "null A, W or C")
    for k in (0, -64, 32, 100, 96):
        refused(L, d(K=k, lda=128), "K=", "multiple of 64")
    refused(L, d(lda=132), "16-byte aligned")
    refused(L, d(K=128, lda=64), "lda=64 < K=128")
    refused(L, d(ldc=39), "ldc=39 < N=40")
    refused(L, d(epi=gm.RESID), "needs resid")
    refused(L, d(epi=gm.RESID, resid=P, ldr=39), "ldr=39 < N=40")
    refused(L, d(epi=16), "unknown epilogue bits")
    refused(L, d(c_kind=3), "c_kind")
    refused(L, d(c_kind=gm.OUT["e4m3"]), "e4m3 output needs e4m3 operands")
    refused(L, d(reserved=1), "reserved")
    refused(L, d(M=-1), "negative")
    refused(L, d(precision=7), "precision must be")
    refused(L, d(precision=K_["CN_PRECISION_FP8"]), "precision must be")
    # a precision of the other library
    refused(L, d(precision=OWN16["f16" if flavour is None else None]), "libcassnat_hip_f16.so")


def test_refusals_of_the_other_element_types():
    L = hip.lib()
    F32, X3, BF16 = K_["CN_PRECISION_F32"], K_["CN_PRECISION_BF16X3"], K_["CN_PRECISION_BF16"]
    for k in (0, 16, 48):
        refused(L, desc(precision=F32, K=k), "multiple of 32")
    refused(L, desc(precision=F32, K=32, lda=34), "16-byte aligned")
    for k in (0, 16, 48):
        refused(L, desc(precision=X3, K=k, lda=64, ldc=64), "multiple of 32")
    refused(L, desc(precision=X3, K=32, lda=48, ldc=64), "split-bf16", "multiples of 32")
    refused(L, desc(precision=X3, K=32, lda=64, ldc=40), "split-bf16", "multiples of 32")
    assert L.cn_gemm_form(C.byref(desc(precision=X3, K=32, lda=64, ldc=40, c_kind=gm.OUT["f32"]))) >= 0  # (an fp32 C has no such need)
    for k in (0, 64, 192):
        refused(L, desc(ab_fp8=1, K=k, lda=256), "multiple of 128")
    refused(L, desc(ab_fp8=1, K=128, lda=136), "16-byte aligned")
    refused(L, desc(ab_fp8=1, K=256, lda=128), "lda=128 < K=256")
    refused(L, desc(ab_fp8=1, precision=F32), "e4m3 operands belong to CN_PRECISION_BF16")
    refused(hip.lib("f16"), desc("f16", ab_fp8=1), "e4m3 operands belong to CN_PRECISION_BF16")
    assert parts(L.cn_gemm_form(C.byref(desc(ab_fp8=1, precision=BF16, c_kind=gm.OUT["e4m3"])))) == (
        gm.ELEM["e4m3"], gm.OUT["e4m3"], gm.TILE["64"])


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_nothing_to_launch_is_not_an_error(flavour):
    L = hip.lib(flavour)
    for kw in (dict(M=0), dict(N=0, ldc=0)):
        d = desc(flavour, **kw)
        assert parts(L.cn_gemm_form(C.byref(d)))[2] == gm.TILE["none"]
        assert L.cn_op_gemm_desc(C.byref(d), None) == 0


def test_cn_op_gemm_still_refuses_what_it_refused():
    L = hip.lib()
    rc = L.cn_op_gemm(0, P, 100, P, None, P, 4, 1, 4, 4, 100, 0, None, 0, None, 1, 1.0, None)
    assert rc != 0 and b"multiple" in L.cn_last_error() and L.cn_last_error().startswith(b"cn_op_gemm: ")
    rc = L.cn_op_gemm(K_["CN_PRECISION_F16"], P, 128, P, None, P, 4, 1, 4, 4, 128, 0, None, 0, None, 1, 1.0, None)
    assert rc != 0 and b"libcassnat_hip_f16.so" in L.cn_last_error()
    rc = L.cn_op_gemm(K_["CN_PRECISION_BF16X3"], P, 48, P, None, P, 4, 1, 4, 4, 32, 0, None, 0, None, 1, 1.0, None)
    assert rc != 0 and b"multiples of 32" in L.cn_last_error()
    # and the new stride checks reach it as they reach the engine's calls
    rc = L.cn_op_gemm(0, P, 32, P, None, P, 3, 1, 4, 4, 32, 0, None, 0, None, 1, 1.0, None)
    assert rc != 0 and b"ldc=3 < N=4" in L.cn_last_error()
    assert L.cn_op_gemm(0, P, 32, P, None, P, 4, 1, 0, 4, 32, 0, None, 0, None, 1, 1.0, None) == 0  # M == 0


# ---- coverage: the non-convolution instantiations of gemm_kernel that gemm.hip compiles (run_form / run_elem / launch_gemm), as
# (element, output, tile).  The fp16 library compiles the same sources, and owns CN_PRECISION_F16 alone (cn_own_precision): its
# 16-bit forms are all it can be asked for.
E, O, T = gm.ELEM, gm.OUT, gm.TILE
INSTANTIATIONS = {
    None: {(e, o, t) for e in (E["fp32"], E["bf16"], E["bf16x3"]) for o in (O["own"], O["f32"]) for t in (T["128"], T["64"], T["fullk"])}
    | {(E["e4m3"], o, t) for o in (O["f32"], O["own"], O["e4m3"]) for t in (T["128"], T["64"])},
    "f16": {(E["fp16"], o, t) for o in (O["own"], O["f32"]) for t in (T["128"], T["64"], T["fullk"])},
}


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_cases_reach_every_instantiation_and_each_runs_the_one_it_claims(flavour):
    L = hip.lib(flavour)
    other = hip.lib("f16" if flavour is None else None)
    reached = set()
    for c, layout in gm.PAIRS:
        d = gm.descriptor(c, layout, lambda name: P)
        mine = gm.LAYOUTS[layout][0] == flavour
        code = (L if mine else other).cn_gemm_form(C.byref(d))
        assert code == gm.form_code(c, layout), (c["name"], layout, parts(code), L.cn_last_error())
        # the query is the authority on which library runs a layout: the other one refuses it
        assert (other if mine else L).cn_gemm_form(C.byref(d)) == -1, (c["name"], layout)
        if mine:
            reached.add(parts(code))
    assert all(t != gm.TILE["linear256"] for _, _, t in reached)
    assert reached == INSTANTIATIONS[flavour], (sorted(INSTANTIATIONS[flavour] - reached), sorted(reached - INSTANTIATIONS[flavour]))


@pytest.mark.parametrize("M, N, tile", [
    (73 * 128, 7 * 128, "64"), (64 * 128, 8 * 128, "128"),          # 511 tiles of 128 x 128: the small tile; 512: the big one
    (511 * 128, 1, "64"), (511 * 128 + 1, 1, "128"),                # ... counted with the ragged last tile
    (1, 511 * 128, "64"), (1, 511 * 128 + 1, "128"),
    (gm.BIG_M, gm.BIG_N, "128"), (gm.BIG_M - 128, gm.BIG_N - 1, "64")])  # 527 and 30 x 16 = 480
def test_the_tile_threshold(M, N, tile):
    L = hip.lib()
    for prec, k, elem in ((K_["CN_PRECISION_F32"], 128, "fp32"), (K_["CN_PRECISION_BF16"], 256, "bf16"), (K_["CN_PRECISION_BF16X3"], 128, "bf16x3")):
        for ksteps, full in ((4, True), (3, False), (5, False)):
            kk = k // 4 * ksteps
            lda = -(-kk // 32) * 32
            d = desc(precision=prec, M=M, N=N, K=kk, lda=lda, ldc=-(-N // 32) * 32)
            want = "128" if tile == "128" else ("fullk" if full else "64")
            assert parts(L.cn_gemm_form(C.byref(d))) == (gm.ELEM[elem], gm.OUT["own"], gm.TILE[want]), (M, N, kk, L.cn_last_error())
    d = desc(ab_fp8=1, M=M, N=N, K=512, lda=512, ldc=N)  # e4m3 operands: 4 slabs take the loop
    assert parts(L.cn_gemm_form(C.byref(d))) == (gm.ELEM["e4m3"], gm.OUT["own"], gm.TILE[tile])


def test_the_linear256_route_is_reported_not_hidden():
    """linear_out's shape class leaves the tiled kernel (test_gpu_frontend.py covers that kernel); the query says so."""
    L = hip.lib()
    d = desc(M=100, N=256, K=1024, lda=1024, ldc=256, c_kind=gm.OUT["f32"], epi=gm.EMBED, pe=P, pe_period=7, scale=16.0)
    assert parts(L.cn_gemm_form(C.byref(d)))[2] == gm.TILE["linear256"]
    d = desc(M=100, N=256, K=1024, lda=1024, ldc=288, c_kind=gm.OUT["f32"], epi=gm.EMBED, pe=P, pe_period=7, scale=16.0)
    assert parts(L.cn_gemm_form(C.byref(d)))[2] == gm.TILE["64"]
