"""The descriptor entry of the subsampling front end (cn_op_frontend_desc) and its argument checks.  No device needed: every call
below must be refused before anything is packed or launched.  The kernels themselves are compared with float64 models in
test_gpu_frontend.py."""
import ctypes as C

import numpy as np
import pytest

from cassnat_asr_public_amd import abi, hip

FLAVOURS = [None, "f16"]
K = abi.CONSTANTS
# a host buffer stands in for every pointer: the calls under test never get as far as reading one (the rows lists are read)
_BUF = np.zeros(1 << 16, np.float32)
P = _BUF.ctypes.data


def own(flavour):
    return K["CN_PRECISION_F16"] if flavour == "f16" else K["CN_PRECISION_BF16"]


def desc(flavour, **kw):
    """A plain 16-bit conv1 launch the entry would accept, with ``kw`` overriding fields."""
    f = dict(precision=own(flavour), conv1_form=K["CN_FE_CONV1_PLAIN"], x=P, w9c=P, bias1=P, B=4, T=20, F=80, C=256, halo=0, img=P,
             img_scale=8.0, img_scale2=1.0, w2=P, bias2=P, c2_out=P, lin_a=P, lin_w=P, lin_bias=P, lin_out=P, M=10, K=1024, lda=1024,
             a_scale=8.0, scale=16.0, pe_period=5)
    f.update(kw)
    return hip.CnFrontendDesc(**f)


def refused(L, d, *words):
    rc = L.cn_op_frontend_desc(C.byref(d) if d is not None else None, None)
    msg = L.cn_last_error().decode()
    assert rc != 0, msg
    assert msg.startswith("cn_op_frontend_desc: "), msg
    for w in words:
        assert w in msg, (w, msg)


def rows(*v):
    return (C.c_int32 * len(v))(*v)


def test_descriptor_entry_is_declared_exported_and_sized_like_the_c_struct():
    names = hip.declared_symbols()
    for name in ("cn_op_frontend_desc", "cn_frontend_desc_size", "cn_op_conv1", "cn_op_conv2", "cn_op_conv_frontend_fp8"):
        assert name in names
        for flavour in FLAVOURS:
            getattr(hip.lib(flavour), name)
    for flavour in FLAVOURS:
        assert hip.lib(flavour).cn_frontend_desc_size() == C.sizeof(hip.CnFrontendDesc) == 208
    assert [n for n, _ in hip.CnFrontendDesc._fields_] == [
        "precision", "conv1_form", "conv2_form", "linear_form", "x", "w9c", "bias1", "B", "T", "F", "C", "halo", "n_sub", "img_scale",
        "img_scale2", "sub_rows", "sub_frames", "meta_out", "img", "w2", "bias2", "c2_out", "out8_scale", "lda", "lin_a", "lin_w", "lin_bias",
        "lin_out", "M", "K", "a_scale", "scale", "pe", "pe_period", "reserved", "q8_out"]
    assert [K["CN_FE_CONV1_" + n] for n in ("PLAIN", "PLANES", "MIXPLANES", "F8_VALU", "F8_MFMA", "BF16_MFMA")] == [1, 2, 3, 4, 5, 6]
    assert [K["CN_FE_CONV2_" + n] for n in ("GENERIC", "DMA", "X3", "MIX", "F8")] == [1, 2, 3, 4, 5]
    assert [K["CN_FE_LINEAR_" + n] for n in ("GENERIC", "DMA", "F8")] == [1, 2, 3]


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refuses_what_the_issue_lists(flavour):
    L = hip.lib(flavour)
    refused(L, None, "null descriptor")
    refused(L, desc(flavour, conv1_form=0), "no stage")
    # a form (or precision) its library does not have
    if flavour == "f16":
        for kw in (dict(conv1_form=K["CN_FE_CONV1_MIXPLANES"], halo=1), dict(conv1_form=K["CN_FE_CONV1_PLANES"], halo=1),
                   dict(conv1_form=K["CN_FE_CONV1_F8_VALU"], halo=1), dict(conv1_form=K["CN_FE_CONV1_F8_MFMA"], halo=1),
                   dict(conv1_form=0, conv2_form=K["CN_FE_CONV2_MIX"], halo=1), dict(conv1_form=0, conv2_form=K["CN_FE_CONV2_X3"], halo=1),
                   dict(conv1_form=0, conv2_form=K["CN_FE_CONV2_F8"], halo=1), dict(conv1_form=0, linear_form=K["CN_FE_LINEAR_F8"], K=5120, lda=5120)):
            refused(L, desc(flavour, **kw), "half-precision library")
        for p in ("F32", "BF16", "BF16X3", "FP8"):
            refused(L, desc(flavour, precision=K["CN_PRECISION_" + p]), "libcassnat_hip_f16.so")
    else:
        refused(L, desc(flavour, precision=K["CN_PRECISION_F16"]), "libcassnat_hip_f16.so")
        refused(L, desc(flavour, precision=K["CN_PRECISION_FP8"]), "precision")
    # a form whose shape rule fails
    for form in ("F8_MFMA", "BF16_MFMA"):
        if flavour == "f16" and form == "F8_MFMA":
            continue
        refused(L, desc(flavour, conv1_form=K["CN_FE_CONV1_" + form], halo=1, C=128), "matrix-core", "C == 256")
        refused(L, desc(flavour, conv1_form=K["CN_FE_CONV1_" + form], halo=1, F=58), "matrix-core", "F1 + 2")
        refused(L, desc(flavour, conv1_form=K["CN_FE_CONV1_" + form], halo=1, F=127), "matrix-core", "F1 + 2")
    refused(L, desc(flavour, conv1_form=0, conv2_form=K["CN_FE_CONV2_DMA"], halo=1, C=128), "LDS-DMA conv2", "C == 256")
    refused(L, desc(flavour, conv1_form=0, conv2_form=K["CN_FE_CONV2_GENERIC"], halo=1, C=128), "bordered image")
    refused(L, desc(flavour, conv1_form=0, linear_form=K["CN_FE_LINEAR_DMA"], K=96, lda=96), "LDS-DMA linear")
    if flavour != "f16":
        for form in ("X3", "MIX", "F8"):
            refused(L, desc(flavour, conv1_form=0, conv2_form=K["CN_FE_CONV2_" + form], halo=1, C=128), "C == 256")
        refused(L, desc(flavour, conv1_form=0, linear_form=K["CN_FE_LINEAR_F8"], K=1024), "5120")
        refused(L, desc(flavour, precision=K["CN_PRECISION_F32"], conv1_form=0, conv2_form=K["CN_FE_CONV2_DMA"], halo=1), "LDS-DMA conv2")
        refused(L, desc(flavour, precision=K["CN_PRECISION_F32"], conv1_form=K["CN_FE_CONV1_BF16_MFMA"], halo=1), "16-bit precision")
    # halo 2 on a form without a border of its own to skip; halo 0 on an always-bordered form; X3 precision with a halo
    refused(L, desc(flavour, conv1_form=K["CN_FE_CONV1_BF16_MFMA"], halo=2), "halo", "matrix-core")
    refused(L, desc(flavour, conv1_form=K["CN_FE_CONV1_BF16_MFMA"], halo=0), "halo", "matrix-core")
    refused(L, desc(flavour, halo=3), "halo is 0, 1 or 2")
    if flavour != "f16":
        refused(L, desc(flavour, conv1_form=K["CN_FE_CONV1_F8_MFMA"], halo=2), "halo", "matrix-core")
        for form in ("PLANES", "MIXPLANES", "F8_VALU"):
            refused(L, desc(flavour, conv1_form=K["CN_FE_CONV1_" + form], halo=0), "always bordered")
        for halo in (1, 2):
            refused(L, desc(flavour, precision=K["CN_PRECISION_BF16X3"], halo=halo), "split-bf16", "no halo")
    refused(L, desc(flavour, conv1_form=0, conv2_form=K["CN_FE_CONV2_DMA"], halo=0), "halo 0", "bordered")
    # a rows list that does not sum to B, or has more than CN_MAX_SUB entries
    r12, r22, r40, f20, f21, f0 = rows(1, 2), rows(2, 2), rows(4, 0), rows(20, 20), rows(20, 21), rows(0, 20)
    adr = C.addressof
    refused(L, desc(flavour, n_sub=2, sub_rows=adr(r12), sub_frames=adr(f20)), "sums to 3", "B = 4")
    refused(L, desc(flavour, n_sub=65, sub_rows=P, sub_frames=P), "at most 64")
    refused(L, desc(flavour, n_sub=-1), "at most 64")
    refused(L, desc(flavour, n_sub=2, sub_rows=adr(r22), sub_frames=adr(f21)), "frames <= T")
    refused(L, desc(flavour, n_sub=2, sub_rows=adr(r22), sub_frames=adr(f0)), "frames <= T")
    refused(L, desc(flavour, n_sub=2, sub_rows=adr(r40), sub_frames=adr(f20)), "rows >= 1")
    refused(L, desc(flavour, n_sub=1), "sub_rows")


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refuses_bad_geometry_missing_pointers_and_stages_that_do_not_fit(flavour):
    L = hip.lib(flavour)
    for kw in (dict(B=0), dict(T=0), dict(F=0), dict(C=0), dict(C=60), dict(C=48)):
        refused(L, desc(flavour, **kw), "channel count")
    refused(L, desc(flavour, B=1 << 20, T=4000), "2^31")
    for name in ("x", "w9c", "bias1"):
        refused(L, desc(flavour, **{name: None}), "conv1 needs")
    refused(L, desc(flavour, img=None), "null img")
    refused(L, desc(flavour, conv1_form=7), "unknown form")
    refused(L, desc(flavour, conv1_form=0, conv2_form=6), "unknown form")
    refused(L, desc(flavour, conv1_form=0, linear_form=-1), "unknown form")
    g = K["CN_FE_CONV2_GENERIC"]
    for name in ("w2", "bias2", "c2_out"):
        refused(L, desc(flavour, conv1_form=0, conv2_form=g, **{name: None}), "conv2 needs")
    # conv2 must read what conv1 writes
    refused(L, desc(flavour, conv2_form=K["CN_FE_CONV2_DMA"], halo=0), "halo 0")
    if flavour != "f16":
        refused(L, desc(flavour, conv2_form=K["CN_FE_CONV2_X3"], halo=1), "does not read")
        refused(L, desc(flavour, conv1_form=K["CN_FE_CONV1_PLANES"], conv2_form=K["CN_FE_CONV2_DMA"], halo=1), "does not read")
        refused(L, desc(flavour, conv1_form=K["CN_FE_CONV1_F8_VALU"], conv2_form=K["CN_FE_CONV2_MIX"], halo=1), "does not read")
        refused(L, desc(flavour, conv1_form=K["CN_FE_CONV1_F8_VALU"], halo=1, img_scale=0.0), "img_scale")
        refused(L, desc(flavour, conv1_form=0, linear_form=K["CN_FE_LINEAR_F8"], K=5120, lda=5184), "lda == K")
    for name in ("lin_a", "lin_w", "lin_bias", "lin_out"):
        refused(L, desc(flavour, conv1_form=0, linear_form=K["CN_FE_LINEAR_DMA"], **{name: None}), "linear needs")
    refused(L, desc(flavour, conv1_form=0, linear_form=K["CN_FE_LINEAR_DMA"], lda=1000), "lda >= K")
    refused(L, desc(flavour, conv1_form=0, linear_form=K["CN_FE_LINEAR_DMA"], pe_period=0), "pe_period")
    refused(L, desc(flavour, conv1_form=0, linear_form=K["CN_FE_LINEAR_DMA"], M=0), "M, K >= 1")
    refused(L, desc(flavour, conv1_form=0, linear_form=K["CN_FE_LINEAR_DMA"], lda=1028), "16-byte")
    refused(L, desc(flavour, conv1_form=0, linear_form=K["CN_FE_LINEAR_GENERIC"], K=1028, lda=1028), "multiples of 8")
