"""Argument checks of the convolution module's kernel entries (cn_op_glu, cn_op_dwconv, cn_op_groupnorm_swish) and cn_model_create's
check of the conformer kernel sizes.  No device needed: every call below must be refused before anything is launched or allocated.  The
kernels themselves are compared with float64 models in test_gpu_convmodule.py."""
import ctypes as C

import numpy as np
import pytest

from cassnat_asr_public_amd import hip

FLAVOURS = [None, "f16"]
# a host buffer stands in for every device pointer: the calls under test never get as far as reading one
_BUF = np.zeros(1 << 16, np.float32)
P = C.c_void_p(_BUF.ctypes.data)
NAMES = ("cn_op_glu", "cn_op_dwconv", "cn_op_groupnorm_swish")


def refused(L, rc, *words):
    msg = L.cn_last_error().decode()
    assert rc != 0, msg
    for w in words:
        assert w in msg, (w, msg)


def precisions(flavour):
    """(precision, split-bf16?) of every layout the library holds."""
    if flavour == "f16":
        return [(hip.PRECISION["fp16"], False)]
    return [(hip.PRECISION["fp32"], False), (hip.PRECISION["bf16"], False), (hip.PRECISION["bf16x3"], True)]


def glu(L, prec, M=4, d=64, src=P, dst=P):
    return L.cn_op_glu(prec, src, dst, M, d, None)


def dwconv(L, prec, B=2, Lf=8, d=64, k=7, form=0, ptrs=(P, P, P, P)):
    return L.cn_op_dwconv(prec, *ptrs, B, Lf, d, k, form, None)


def gnorm(L, prec, B=2, Lf=8, d=64, ptrs=(P, P, P, P, P)):
    return L.cn_op_groupnorm_swish(prec, *ptrs, B, Lf, d, 1e-5, None)


def test_entries_are_declared_exported_and_typed():
    names = hip.declared_symbols()
    for name in NAMES:
        assert name in names
        for flavour in FLAVOURS:
            fn = getattr(hip.lib(flavour), name)
            assert fn.argtypes is not None and fn.restype is C.c_int
    for flavour in FLAVOURS:
        Lb = hip.lib(flavour)
        assert len(Lb.cn_op_glu.argtypes) == 6 and len(Lb.cn_op_dwconv.argtypes) == 11 and len(Lb.cn_op_groupnorm_swish.argtypes) == 11


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refuse_the_other_builds_precision(flavour):
    L = hip.lib(flavour)
    other = hip.PRECISION["bf16" if flavour == "f16" else "fp16"]
    word = "CN_PRECISION_F16" if flavour == "f16" else "libcassnat_hip_f16"
    refused(L, glu(L, other), "cn_op_glu", word)
    refused(L, dwconv(L, other), "cn_op_dwconv", word)
    refused(L, gnorm(L, other), "cn_op_groupnorm_swish", word)
    if flavour is None:  # (the fp8 engine stores bf16: it has no layout of its own)
        refused(L, glu(L, hip.PRECISION["fp8"]), "precision must be")


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refuse_null_pointers(flavour):
    L = hip.lib(flavour)
    for prec, _ in precisions(flavour):
        refused(L, glu(L, prec, src=None), "cn_op_glu", "null pointer")
        refused(L, glu(L, prec, dst=None), "cn_op_glu", "null pointer")
        for i in range(4):
            refused(L, dwconv(L, prec, ptrs=tuple(None if j == i else P for j in range(4))), "cn_op_dwconv", "null pointer")
        for i in range(5):
            refused(L, gnorm(L, prec, ptrs=tuple(None if j == i else P for j in range(5))), "cn_op_groupnorm_swish", "null pointer")


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refuse_sizes_below_one(flavour):
    L = hip.lib(flavour)
    for prec, _ in precisions(flavour):
        for bad in (0, -1):
            refused(L, glu(L, prec, M=bad), "M and d must be >= 1")
            refused(L, glu(L, prec, d=bad), "M and d must be >= 1")
            for name in ("B", "Lf", "d", "k"):
                refused(L, dwconv(L, prec, **{name: bad}), "B, L, d and k must be >= 1")
            for name in ("B", "Lf", "d"):
                refused(L, gnorm(L, prec, **{name: bad}), "B, L and d must be >= 1")
        refused(L, dwconv(L, prec, form=2), "form must be 0")
        refused(L, dwconv(L, prec, form=-1), "form must be 0")


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refuse_images_beyond_int_arithmetic(flavour):
    """The kernels index an utterance's L x d image (the GLU: a row of 2 d) and the B L rows with int."""
    L = hip.lib(flavour)
    big = 1 << 16
    for prec, _ in precisions(flavour):
        refused(L, glu(L, prec, M=big, d=big), "cn_op_glu", "int arithmetic")  # M * 2d = 2^33
        refused(L, glu(L, prec, M=1 << 14, d=big), "cn_op_glu", "int arithmetic")  # M * 2d = 2^31
        refused(L, dwconv(L, prec, B=1, Lf=big, d=big), "cn_op_dwconv", "int arithmetic")
        refused(L, dwconv(L, prec, B=1, Lf=1 << 15, d=big), "cn_op_dwconv", "int arithmetic")  # L * d = 2^31
        refused(L, dwconv(L, prec, B=big, Lf=1 << 15, d=32), "cn_op_dwconv", "int arithmetic")  # B * L = 2^31
        refused(L, dwconv(L, prec, B=1 << 10, Lf=1 << 14, d=big), "cn_op_dwconv", "int arithmetic")  # 2^40 elements
        refused(L, dwconv(L, prec, B=1, Lf=1, d=big, k=1 << 15), "cn_op_dwconv", "d * k")
        refused(L, gnorm(L, prec, B=1, Lf=big, d=big), "cn_op_groupnorm_swish", "int arithmetic")
        refused(L, gnorm(L, prec, B=1, Lf=1 << 15, d=big), "cn_op_groupnorm_swish", "int arithmetic")
        refused(L, gnorm(L, prec, B=big, Lf=1 << 15, d=32), "cn_op_groupnorm_swish", "int arithmetic")


def test_refuse_split_rows_that_are_no_whole_groups_of_32():
    L = hip.lib()
    x3 = hip.PRECISION["bf16x3"]
    for d in (1, 31, 48, 144, 255):
        refused(L, glu(L, x3, d=d), "cn_op_glu", "d % 32")
        refused(L, dwconv(L, x3, d=d), "cn_op_dwconv", "d % 32")
        refused(L, gnorm(L, x3, d=d), "cn_op_groupnorm_swish", "d % 32")


def config(**kw):
    f = dict(input_size=80, d_model=128, n_head=2, d_encff=256, d_decff=256, n_enc=2, n_extra=0, n_self_dec=1, n_mix_dec=2, vocab_size=40,
             max_batch=2, max_frames=64, device=0, enc_max_rel=5, dec_max_rel=3, enc_kernel=7, dec_kernel=3)
    f.update(kw)
    return hip.CnConfig(**f)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_model_create_refuses_even_conformer_kernel_sizes(flavour):
    """The reference's Conv1d(padding = (k - 1) // 2) yields L - 1 frames for an even k and its residual add fails; the engine would compute
    L frames with a lopsided window.  Refused where the configuration is validated, before a device is touched."""
    L = hip.lib(flavour)
    prec = hip.PRECISION["fp16" if flavour == "f16" else "fp32"]
    for bad in (4, 30, 0, -3):
        for field, flags in (("enc_kernel", dict(conf_enc=1)), ("enc_kernel", dict(conf_enc=1, conf_dec=1)), ("enc_kernel", dict(conf_enc=1, ast=1)),
                             ("dec_kernel", dict(conf_dec=1)), ("dec_kernel", dict(conf_enc=1, conf_dec=1))):
            h = C.c_void_p()
            rc = L.cn_model_create(C.byref(config(precision=prec, **{field: bad}, **flags)), C.byref(h))
            assert not h.value
            refused(L, rc, "cn_model_create", field, "odd")
