"""The float64 models of the convolution module's kernels (convmodule_model.py) - no device needed.  At the very cases the GPU test runs
(test_gpu_convmodule.py): the models, composed, are the oracle's ConvModule; a float32 emulation of each kernel's arithmetic as written
stays within half the bound; and every mistake of MISTAKES moves some element by twice the bound or more in every layout, so the GPU gates
would catch a kernel that made it.

The emulation's float32 result is compared with the bound WITHOUT the layout's output rounding (the model asked for the fp32 layout on
the layout's operands): the rounding of a stored bf16 / fp16 element alone reaches half an ulp, which is the whole of that term, so only
the arithmetic part can be held to 0.5.  The rounded emulation is held to the full bound."""
import pytest
import torch

import convmodule_model as cm
from attention_model import LAYOUTS, round_operand, to_layout
from oracle import conformer_oracle

LAYOUT_NAMES = list(LAYOUTS)


def operand(x, layout):
    return to_layout(x, layout, device="cpu")[1]


def ratio(got, ref, bound):
    return float(((got.double() - ref).abs() / bound).max())


# ============================================================================================ the models are the oracle's module
@pytest.mark.parametrize("B,L,d,k", [(2, 9, 32, 5), (3, 33, 64, 15), (2, 5, 32, 31)])
def test_models_composed_equal_the_oracle_conv_module(B, L, d, k):
    """conv_module in float64 with identity pointwise convolutions: ties [B L][d] and [d][k] to torch's (B, C, T) and (C, 1, k), the
    padding to (k - 1) // 2 on both sides, and the statistics to the whole image of an utterance."""
    g = torch.Generator().manual_seed(k)
    x = torch.randn(B, L, 2 * d, generator=g, dtype=torch.float64)
    x[1] = x[1] * 3 + 1
    w = torch.randn(d, k, generator=g, dtype=torch.float64)
    bias, gw, gb = (torch.randn(d, generator=g, dtype=torch.float64) for _ in range(3))
    st = {"m.pointwise_conv1.weight": torch.eye(2 * d, dtype=torch.float64)[:, :, None], "m.pointwise_conv1.bias": torch.zeros(2 * d, dtype=torch.float64),
          "m.depthwise_conv.weight": w[:, None, :], "m.depthwise_conv.bias": bias, "m.norm.weight": gw, "m.norm.bias": gb,
          "m.pointwise_conv2.weight": torch.eye(d, dtype=torch.float64)[:, :, None], "m.pointwise_conv2.bias": torch.zeros(d, dtype=torch.float64)}
    want = conformer_oracle.conv_module(st, "m", x).reshape(B * L, d)
    a, _ = cm.glu_model(x.reshape(B * L, 2 * d), "fp32")
    y, _ = cm.dwconv_model(a, w, bias, B, L, k)
    got, _, _, _ = cm.groupnorm_swish_model(y, gw, gb, B, L, 1e-5, "fp32")
    assert float(((got - want).abs() / want.abs().clamp(min=1.0)).max()) < 1e-12
    assert float(((got - want).abs().max() / want.abs().max())) < 1e-12


# ============================================================================================ the arithmetic as written is inside the bound
@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_glu_emulation_within_half_the_bound(layout):
    for M, d in cm.GLU_SHAPES:
        if layout == "bf16x3" and not cm.splits(d):
            continue
        x = operand(cm.glu_case(M, d), layout)
        emu = cm.glu_emulation(x)
        ref, arith = cm.glu_model(x, "fp32")
        assert ratio(emu, ref, arith) <= 0.5, (M, d)
        _, bound = cm.glu_model(x, layout)
        assert ratio(round_operand(emu, layout), ref, bound) <= 1.0, (M, d)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("k", cm.DW_TILED_K + cm.DW_NAIVE_K)
def test_dwconv_emulation_within_half_the_bound(layout, k):
    for L, d in cm.dw_shapes(k):
        if layout == "bf16x3" and not cm.splits(d):
            continue
        _, _, _, x, w, bias, ref, bound = cm.dw_reference(layout, k, L, d)
        assert ratio(cm.dwconv_emulation(x, w, bias, cm.DW_B, L, k), ref, bound) <= 0.5, (L, d)


@pytest.mark.parametrize("i", range(len(cm.GN_SHAPES)))
def test_groupnorm_swish_emulation_within_half_the_bound(i):
    (B, L, d), kinds = cm.GN_SHAPES[i]
    _, _, _, x, gw, gb, stats = cm.gn_reference(i)
    emu = cm.groupnorm_swish_emulation(x, gw, gb, B, L, cm.GN_EPS)
    ref, arith, _, stats_bound = cm.groupnorm_swish_model(x, gw, gb, B, L, cm.GN_EPS, "fp32", stats=stats)
    assert ratio(emu, ref, arith) <= 0.5, kinds
    img = x.reshape(B, L * d)
    sums = torch.stack([img.sum(1), (img * img).sum(1)], 1)  # (double sums in torch's order)
    assert ratio(sums, stats, stats_bound) <= 0.5
    for b, kind in enumerate(kinds):
        if kind == "const":  # zero variance: swish(beta[c]) within the bound
            sw = (gb * torch.sigmoid(gb))[None].expand(L, d)
            assert ((ref[b * L:(b + 1) * L] - sw).abs() <= arith[b * L:(b + 1) * L]).all()
    for layout in LAYOUT_NAMES:
        if layout == "bf16x3" and not cm.splits(d):
            continue
        _, bound, _, _ = cm.groupnorm_swish_model(x, gw, gb, B, L, cm.GN_EPS, layout, stats=stats)
        assert ratio(round_operand(emu, layout), ref, bound) <= 1.0, (layout, kinds)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
def test_sequence_emulation_within_the_composed_bound(layout):
    """The three emulations chained as the device chains them (GLU stored in the layout, the convolution in float32)."""
    B, L, d, k = (cm.SEQ_SHAPE[n] for n in ("B", "L", "d", "k"))
    x, w, bias, gw, gb = cm.seq_case()
    x = operand(x, layout)
    w, bias, gw, gb = w.double(), bias.double(), gw.double(), gb.double()
    g = round_operand(cm.glu_emulation(x), layout)
    y = cm.dwconv_emulation(g, w, bias, B, L, k).double()
    emu = round_operand(cm.groupnorm_swish_emulation(y, gw, gb, B, L, cm.GN_EPS), layout)
    ref, bound = cm.conv_module_model(x, w, bias, gw, gb, B, L, k, cm.GN_EPS, layout)
    assert ratio(emu, ref, bound) <= 1.0


# ============================================================================================ the bounds can fail
def worst_overshoot(pairs):
    """max over cases and elements of |wrong - right| / bound."""
    return max(float(((wrong - ref).abs() / bound).max()) for ref, bound, wrong in pairs)


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("mistake", [m for m in cm.MISTAKES if m.startswith("glu_")])
def test_glu_bound_catches(layout, mistake):
    def pairs():
        for M, d in cm.GLU_SHAPES:
            if layout == "bf16x3" and not cm.splits(d):
                continue
            x = operand(cm.glu_case(M, d), layout)
            yield cm.glu_model(x, layout) + (cm.glu_model(x, layout, mistakes=(mistake,))[0],)
    assert worst_overshoot(pairs()) >= 2.0


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("mistake", [m for m in cm.MISTAKES if m.startswith("dw_")])
def test_dwconv_bound_catches(layout, mistake):
    """Per kernel size: each size has its own kernel instance (or, on the naive kernel, its own loop count), so each must have a case that
    catches the mistake - but for what a size cannot get wrong: one tap has no order and no transposed reading."""
    for k in cm.DW_TILED_K + cm.DW_NAIVE_K:
        if k == 1 and mistake in ("dw_taps_flipped", "dw_weight_transposed", "dw_leaks_across_utterances", "dw_last_tile_short"):
            continue

        def pairs():
            for L, d in cm.dw_shapes(k):
                if layout == "bf16x3" and not cm.splits(d):
                    continue
                _, _, _, x, w, bias, ref, bound = cm.dw_reference(layout, k, L, d)
                yield ref, bound, cm.dwconv_model(x, w, bias, cm.DW_B, L, k, mistakes=(mistake,))[0]
        assert worst_overshoot(pairs()) >= 2.0, k


@pytest.mark.parametrize("layout", LAYOUT_NAMES)
@pytest.mark.parametrize("mistake", [m for m in cm.MISTAKES if m.startswith("gn_")])
def test_groupnorm_swish_bound_catches(layout, mistake):
    def pairs():
        for i, ((B, L, d), _) in enumerate(cm.GN_SHAPES):
            if layout == "bf16x3" and not cm.splits(d):
                continue
            _, _, _, x, gw, gb, stats = cm.gn_reference(i)
            ref, bound, _, _ = cm.groupnorm_swish_model(x, gw, gb, B, L, cm.GN_EPS, layout, stats=stats)
            yield ref, bound, cm.groupnorm_swish_model(x, gw, gb, B, L, cm.GN_EPS, layout, mistakes=(mistake,), stats=stats)[0]
    assert worst_overshoot(pairs()) >= 2.0


def test_every_mistake_has_a_test():
    assert all(m.split("_")[0] in ("glu", "dw", "gn") for m in cm.MISTAKES) and len(set(cm.MISTAKES)) == 14
