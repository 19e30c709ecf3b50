"""Argument checks of the AST beam search's kernel entries (no device needed: every call below must be refused before anything
is launched).  The kernels themselves are compared with float64 models in test_gpu_ast_kernels.py."""
import ctypes as C

import numpy as np
import pytest

from cassnat_asr_public_amd import hip

FLAVOURS = [None, "f16"]
# a host buffer stands in for every device pointer: the calls under test never get as far as reading one
_BUF = np.zeros(1 << 16, np.float32)
P = C.c_void_p(_BUF.ctypes.data)


def refused(L, rc, *words):
    msg = L.cn_last_error().decode()
    assert rc != 0, msg
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_topk_launchers_refuse_k_above_the_vocabulary(flavour):
    """k > V: a selection round would pick an already retired -inf entry again (or write index 0x7fffffff); torch.topk raises."""
    L = hip.lib(flavour)
    refused(L, L.cn_op_logsoftmax_topk(P, 2, 20, 1.0, 21, P, P, None), "min(32, V)")
    refused(L, L.cn_op_logsoftmax_fuse_topk(P, P, 2, 20, 1.0, 0.5, 21, P, P, None), "min(32, V)")
    refused(L, L.cn_op_topk(P, 2, 20, 21, P, P, None), "min(64, V)")
    refused(L, L.cn_op_logsoftmax_fuse_topk(P, P, 2, 8193, 1.0, 0.5, 4, P, P, None), "8192")
    refused(L, L.cn_op_logsoftmax_fuse_topk(P, P, 2, 40, 1.0, 0.5, 33, P, P, None), "32")
    refused(L, L.cn_op_logsoftmax_gather(P, 2, 40, P, 257, P, None), "256")
    refused(L, L.cn_op_logsoftmax_gather(P, 2, 16385, P, 4, P, None), "16384")


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_ctc_prefix_refuses_out_len_beyond_the_frames(flavour):
    """out_len > Tp: the kernel's first loop would write states past the candidate's Tp x 2 block (the reference raises IndexError)."""
    L = hip.lib(flavour)
    for Tp, out_len in ((7, 8), (1, 2), (61, 100), (9, -1)):
        refused(L, L.cn_op_ast_ctc_prefix(*[P] * 9, 3, 4, Tp, 40, 0, 2, out_len, None), "out_len <= Tp")
    refused(L, L.cn_op_ast_ctc_prefix(*[P] * 9, 3, 4, 7, 40, 40, 2, 3, None), "blank < V")
    refused(L, L.cn_op_ast_ctc_prepare(P, P, P, 2, 0, 40, 0, None), "Tp")


def beam_update(L, bw, K, B=1, cur=0):
    return L.cn_op_ast_beam_update(*[P] * 23, cur, 0, bw, K, 8, 2, 1, 0, 1, 1, 0, 0.5, 0.5, 0.0, 0.0, B, None)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_beam_kernels_refuse_widths_outside_1_to_32(flavour):
    L = hip.lib(flavour)
    for bw, K in ((0, 5), (33, 33), (1, 33), (3, 0), (5, 4), (32, 31)):
        refused(L, beam_update(L, bw, K), "beam_width <= K <= 32")
    refused(L, beam_update(L, 3, 5, cur=2), "cur 0 or 1")
    refused(L, beam_update(L, 3, 5, B=0), "B >= 1")
    for bw in (0, 33):
        refused(L, L.cn_op_ast_beam_init(*[P] * 19, 0, 1, bw, 8, 1, 0, None), "beam_width <= 32")
    refused(L, L.cn_op_ast_beam_update(*[P] * 18, None, *[P] * 4, 0, 0, 3, 5, 8, 2, 1, 0, 1, 1, 0, 0.5, 0.5, 0.0, 0.0, 1, None),
            "null state array")


def gather_attn(L, prec, mode, ldq, ldo, H=2, d=128, nkeys=10, slots=4, table_stride=10, append_pos=-1, n=4):
    return L.cn_op_ast_gather_attn(prec, mode, P, ldq, P, P, P, ldo, n, H, nkeys, slots, d, table_stride, P, P, P, P, 0.125,
                                   append_pos, None)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_gather_attention_refuses_bad_geometry(flavour):
    L = hip.lib(flavour)
    f32, x3 = hip.PRECISION["fp32"], hip.PRECISION["bf16x3"]
    own16 = hip.PRECISION["fp16" if flavour == "f16" else "bf16"]
    other16 = hip.PRECISION["bf16" if flavour == "f16" else "fp16"]
    if flavour == "f16":  # the half-precision build holds the 16-bit layout only
        refused(L, gather_attn(L, f32, 0, 384, 128), "CN_PRECISION_F16")
    else:  # split-bf16 rows: strides must be whole groups of 32 elements
        refused(L, gather_attn(L, x3, 0, 384 + 16, 128), "multiples of 32")
        refused(L, gather_attn(L, x3, 1, 128, 128 + 8), "multiples of 32")
        refused(L, gather_attn(L, hip.PRECISION["fp8"], 0, 384, 128), "precision must be")
    refused(L, gather_attn(L, other16, 0, 384, 128), "F16")
    refused(L, gather_attn(L, own16, 0, 384, 128, H=2, d=96), "d = 64 * H")
    refused(L, gather_attn(L, own16, 2, 384, 128), "mode")
    refused(L, gather_attn(L, own16, 0, 384, 128, H=17, d=17 * 64), "H <= 16")
    refused(L, gather_attn(L, own16, 0, 2 * 128, 128), "ldq >= 3d")
    refused(L, gather_attn(L, own16, 1, 128, 64), "ldo >= d")
    refused(L, gather_attn(L, own16, 0, 384, 128, nkeys=0), "nkeys >= 1")
    refused(L, gather_attn(L, own16, 0, 384, 128, append_pos=10), "append_pos < nkeys")
    refused(L, gather_attn(L, own16, 0, 384, 128, slots=3), "slots >= n")
    refused(L, gather_attn(L, own16, 0, 384, 128, table_stride=9), "table_stride >= nkeys")
    # 64 KB of scores per workgroup: H * nkeys <= 16384
    refused(L, gather_attn(L, own16, 1, 128, 128, nkeys=8193, slots=4, table_stride=8193), "score buffer")


def gather_attn_rows(L, prec, H=2, d=128, ldq=384, ldo=128, table_stride=10, max_keys=10, rowid=P, pos=P, stay=P, n=4):
    return L.cn_op_ast_gather_attn_rows(prec, P, ldq, P, P, P, ldo, n, H, d, table_stride, max_keys, rowid, pos, stay, 0.125, None)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_gather_attention_rows_refuses_bad_geometry(flavour):
    L = hip.lib(flavour)
    own16 = hip.PRECISION["fp16" if flavour == "f16" else "bf16"]
    refused(L, gather_attn_rows(L, hip.PRECISION["bf16" if flavour == "f16" else "fp16"]), "F16")
    refused(L, gather_attn_rows(L, own16, table_stride=9), "table_stride >= max_keys")
    for missing in ("rowid", "pos", "stay"):
        refused(L, gather_attn_rows(L, own16, **{missing: None}), "tables")
    refused(L, gather_attn_rows(L, own16, H=17, d=17 * 64, ldq=3 * 17 * 64, ldo=17 * 64), "H <= 16")
    refused(L, gather_attn_rows(L, own16, d=96), "d = 64 * H")
    refused(L, gather_attn_rows(L, own16, max_keys=0), "max_keys >= 1")
    refused(L, gather_attn_rows(L, own16, ldq=256), "ldq >= 3d")
    refused(L, gather_attn_rows(L, own16, max_keys=8193, table_stride=8193), "score buffer")
    if flavour != "f16":
        refused(L, gather_attn_rows(L, hip.PRECISION["bf16x3"], ldq=384 + 16), "multiples of 32")
