"""The checks of x3_model.py on the CPU: for every case the emulation (a stand-in for the kernels: the same operation with every
operand and intermediate rounding, float64 accumulation) passes the guards, the per-element bound and the aggregate check; and each
mistake a kernel or its launcher could plausibly make fails, in every case it applies to, by the check named in CAUGHT_BY.  Run
with -s for the smallest aggregate ratio each mistake reaches per family (the figures beside x3_model.RATIO)."""
import pytest

import x3_model as xm

clone = lambda b: {k: v.clone() for k, v in b.items()}

# mistake: the checks that catch it ("untouched": the guards; "bound": |out - fp64| <= bound, which includes a split output's
# halves; "ratio": the aggregate check).  Where "ratio" is named, some cases are caught by the aggregate check alone: the test
# asserts a failure for every case the mistake applies to.
CAUGHT_BY = {
    "w_lo_x_hi_dropped": ("bound", "ratio"), "w_hi_x_lo_dropped": ("bound", "ratio"),
    "out_hi_lo_swapped": ("bound",), "lo_plane_offset": ("untouched",), "halfwave_groups_not_swapped": ("bound", "ratio"),
    "chunk_last_tile_skipped": ("bound",), "tail_tile_shifted": ("bound",),
    "rows_past_M_stored": ("untouched",), "last_row_duplicated": ("bound",),
    "resid_scale_ignored": ("bound",), "resid_read_after_store": ("bound",),
    "no_b1": ("bound", "ratio"), "no_b2": ("bound", "ratio"), "no_bo": ("bound", "ratio"), "no_bt": ("bound", "ratio"),
    "relu_before_bias": ("bound", "ratio"), "swish_as_relu": ("bound",),
    "ln1_biased_std": ("bound", "ratio"), "lnn_eps_in_var": ("bound", "ratio"), "lnn_uses_ln1_vectors": ("bound", "ratio"),
    "mix_l_q_swapped": ("ratio",), "mix_weight_scale_x2": ("ratio",), "mix_act_l_scale_2_10": ("ratio",),
    "mix_q_not_saturated": ("bound",),
}
SMALLEST = {}


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    print("\nsmallest rms(out - fp64) / yardstick a mistake reaches, per family (where the guards do not catch it first):")
    for fam in sorted({f for f, _ in SMALLEST}):
        rows = sorted((r, m) for (f, m), r in SMALLEST.items() if f == fam)
        print(f"  {fam:10s} allowed {xm.RATIO[fam]}: " + ", ".join(f"{m} {r:.2f}" for r, m in rows[:4]))
    xm._MODEL.clear()


def test_the_lists_agree():
    assert set(CAUGHT_BY) == set(xm.MISTAKES)
    assert len({c["name"] for c in xm.CASES}) == len(xm.CASES)
    for m in xm.MISTAKES:
        assert any(xm.applies(m, c) for c in xm.CHEAP), m


@pytest.mark.parametrize("c", xm.CASES, ids=[xm.case_id(c) for c in xm.CASES])
def test_emulation_passes_both_checks(c):
    before = xm.buffers(c)
    after = xm.emulate_launch(c, clone(before))
    seen = {}
    xm.check_launch(c, before, after, seen)
    assert set(seen) == set(xm.outputs(c))
    for name, (bratio, ratio, _) in seen.items():
        assert bratio <= 1.0 and ratio <= 1.0 + 1e-9, (name, bratio, ratio)  # (the emulation IS the yardstick's first term)


def test_the_saturation_term_is_what_covers_the_range_cases():
    """Without the two saturation terms the mixed form's bound does not hold for hidden units beyond 448 (the emulation saturates
    as the kernel does); the split form's cases pass with no such term in their bound.  (LayerNorm outputs beyond 448: three
    channels of 256 saturate there, and the accumulation term of a row that holds 30000 is as large as what they lose - the bound
    without the terms is 1.4 .. 3.4 times smaller and still holds.)"""
    import frontend_model as fm

    for c in xm.CASES:
        if c["kind"] != "ffn" or not c["rng"] or not c["mix"] or c["rng"] not in (("hidden", 1000), ("hidden", 30000)):
            continue
        before = xm.buffers(c)
        after = xm.emulate_launch(c, clone(before))
        xm.check_launch(c, before, after)
        old, xm.E4M3_MAX = xm.E4M3_MAX, float("inf")  # the bound of a format that never saturates
        xm._MODEL.pop(c["name"])
        try:
            with pytest.raises(xm.LaunchError) as e:
                xm.check_launch(c, before, after)
            assert e.value.kind == "bound", c["name"]
        finally:
            xm.E4M3_MAX = old
            xm._MODEL.pop(c["name"], None)
    assert fm.MIX_LG_AL == 11 and fm.MIX_LG_AQ == 0


@pytest.mark.parametrize("mistake", xm.MISTAKES)
def test_mistake_is_caught(mistake):
    tried = 0
    for c in xm.CHEAP:
        if not xm.applies(mistake, c):
            continue
        tried += 1
        before = xm.buffers(c)
        after = xm.emulate_launch(c, clone(before), (mistake,))
        seen = {}
        try:
            xm.check_launch(c, before, after, seen, enforce=False)
            ratio = max(r for _, r, _ in seen.values())
            key = (xm.family(c), mistake)
            SMALLEST[key] = min(SMALLEST.get(key, float("inf")), ratio)
        except xm.LaunchError as e:  # (what raises without enforcing: the guards, an xn_out that is not finite)
            assert e.kind in ("untouched", "bound")
        with pytest.raises(xm.LaunchError) as e:
            xm.check_launch(c, before, after)
        assert e.value.kind in CAUGHT_BY[mistake], (c["name"], e.value.kind, str(e.value))
    assert tried > 0
