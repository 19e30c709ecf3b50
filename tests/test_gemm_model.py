"""The checks of gemm_model.py would catch what the tiled GEMM can get wrong - shown on the CPU, on the case list the GPU test
(test_gpu_gemm.py) runs.  A launch is stood in for by the model's EMULATION (float64 accumulation, the output's rounding) writing
the launch's C:

* the correct emulation passes every case in every layout: the bounds hold, the aggregate ratio is at most 1 by construction,
  nothing outside the launch's own elements is written;
* the emulation with one deliberate mistake fails at least one case - an untouched sentinel, the per-element bound or the
  aggregate check.  The table (-s) names the check, layout and case that catch each mistake first;
* the smallest aggregate ratio a value mistake produces is printed per layout with the mistake's name: RATIO sits below it."""
import pytest
import torch

import gemm_model as gm

FOUND = {}
SMALL = [(c, l) for c, l in gm.PAIRS if c["M"] * c["N"] <= 1 << 20]

# the (case, layout) pairs a mistake can show on
APPLIES = {
    "no_bias": lambda c, l: c["bias"],
    "swish_as_relu": lambda c, l: c["epi"] & gm.SWISH,
    "relu_after_resid": lambda c, l: c["epi"] & gm.RELU and c["epi"] & gm.RESID,
    "scale_on_pe": lambda c, l: c["pe"],
    "pe_unwrapped": lambda c, l: c["pe"] and c["M"] > c["period"],
    "resid_scale_ignored": lambda c, l: c["resid"] and c["resid_scale"] != 1.0,
    "ldr_as_n": lambda c, l: c["resid"] and gm.geometry(c, l)["ldr"] != c["N"],
    "lda_as_k": lambda c, l: c["lda_pad"] > 0,
    "ldc_as_n": lambda c, l: gm.geometry(c, l)["ldc"] != c["N"],
    "last_slab_dropped": lambda c, l: c["tile"] != "fullk",
    "fullk_slab3_dropped": lambda c, l: c["tile"] == "fullk",
    "rows_past_m_stored": lambda c, l: True,
    "cols_past_n_stored": lambda c, l: gm.geometry(c, l)["ldc"] > c["N"],
    "xcd_tiles_swapped": lambda c, l: c["N"] > gm.tile_edge(c),
    "w_inv_ignored": lambda c, l: c["w_inv"],
    "c_scale_before_resid": lambda c, l: c["out"] == "e4m3" and c["resid"],
    "no_saturation": lambda c, l: c["sat"],
    "split_lo_dropped_in": lambda c, l: l == "bf16x3",
    "split_lo_wrong_offset": lambda c, l: gm.geometry(c, l)["okind"] == "split",
}
STORES = ("ldc_as_n", "rows_past_m_stored", "cols_past_n_stored", "split_lo_wrong_offset")  # caught by a sentinel, not by a value


def run(c, layout, mistakes=(), worst=None, enforce=True):
    before = gm.buffers(c, layout)
    after = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in before.items()}
    gm.emulate_launch(c, layout, after, mistakes)
    gm.check_launch(c, layout, before, after, worst, enforce)


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    print("\nmistake: what catches it first per layout (check, case, rms ratio of an aggregate failure)")
    for (name, layout), (kind, case, ratio) in sorted(FOUND.items()):
        print(f"  {name:22s} {layout:6s} {kind:10s} {case:34s} {'' if ratio is None else f'{ratio:.1f}'}")
    gm._MODEL.clear()


def test_every_mistake_has_a_predicate_and_the_case_list_covers_what_the_issue_names():
    assert set(APPLIES) == set(gm.MISTAKES)
    names = [c["name"] for c in gm.CASES]
    assert len(set(names)) == len(names)
    small = [c for c in gm.CASES if c["tile"] != "128" and c["layouts"] == gm.GENERIC]
    assert {1, 63, 64, 65, 129} <= {c["M"] for c in small} and {1, 33, 64, 65, 200} <= {c["N"] for c in small}
    assert any(c["M"] == 65 and c["N"] == 65 for c in small)
    assert {1, 2, 3, 4, 5} <= {c["slabs"] for c in small} and any(c["K"] == 2048 for c in small)
    assert any(c["tile"] == "fullk" and c["lda_pad"] and c["ldc_pad"] for c in small)
    big = [c for c in gm.CASES if c["tile"] == "128"]
    assert all((c["M"], c["N"]) == (gm.BIG_M, gm.BIG_N) and c["ldc_pad"] for c in big)
    assert {c["slabs"] for c in big if c["slabs"]} == {3, 4}
    assert all(c["M"] * c["N"] <= 1 << 20 for c in gm.CASES if c["tile"] != "128")
    # one big case per (element type, output type) at most
    seen = [(layout, c["out"]) for c in big for layout in c["layouts"]]
    assert len(seen) == len(set(seen))
    f8 = [c for c in gm.CASES if c["layouts"] == ("e4m3",)]
    assert {c["K"] for c in f8} >= {128, 256, 2048} and {c["out"] for c in f8} == {"own", "f32", "e4m3"}
    assert any(c["w_inv"] for c in f8) and any(not c["w_inv"] for c in f8) and any(c["sat"] for c in f8)
    # the period of the EMBED case divides neither M nor 64
    for c in gm.CASES:
        if c["pe"]:
            assert c["M"] % c["period"] and 64 % c["period"] and c["M"] > c["period"]


def test_the_e4m3_accumulation_term_stays_inside_what_the_old_test_allows():
    """test_gemm_fp8_matches_an_e4m3_emulation allows 1e-4 of the output range: the accumulation term of every e4m3 case stays
    there (it is capped; the cases the cap binds in are printed), and the constant is twice its measurement."""
    assert gm.E4M3_ACC >= 2 * gm.E4M3_ACC_MEASURED and gm.E4M3_RANGE_CAP == 1e-4
    for c, layout in gm.PAIRS:
        if layout == "e4m3" and c["M"] * c["N"] <= 1 << 20:
            b = gm.buffers(c, layout)
            o = gm.operands(c, layout, b)
            res = gm.gemm_model(dict(c, epi=0, resid=None, out="f32"), layout, o)  # the product and its bias alone
            rng = float(res["ref"].abs().max())
            assert float(res["f8_term"].max()) <= 1e-4 * rng * (1 + 1e-12), c["name"]
            over = float((gm.E4M3_ACC * res["S"]).max()) / (1e-4 * rng)
            if over > 1:
                print(f"{c['name']}: E4M3_ACC sum |a| |w| deq reaches {over:.2f} x 1e-4 of the output range: capped")


def test_the_emulation_alone_passes_every_case():
    for c, layout in gm.PAIRS:
        worst = {}
        run(c, layout, worst=worst)
        assert worst["rms"] <= 1.0 + 1e-9, (c["name"], layout, worst)


@pytest.mark.parametrize("mistake", gm.MISTAKES)
def test_mistake_is_caught(mistake):
    pairs = [(c, l) for c, l in SMALL if APPLIES[mistake](c, l)]
    assert pairs, "no case of the GPU test can show this mistake"
    layouts = sorted({l for _, l in pairs})
    caught = {}
    for c, layout in pairs:
        if layout in caught:
            continue
        try:
            run(c, layout, (mistake,))
        except gm.LaunchError as e:
            caught[layout] = FOUND[(mistake, layout)] = (e.kind, c["name"], e.ratio)
    assert sorted(caught) == layouts, f"{mistake}: no case catches it in {sorted(set(layouts) - set(caught))}"
    if mistake in STORES:
        assert all(kind == "untouched" for kind, _, _ in caught.values()), caught


def test_a_dropped_lo_half_is_caught_by_the_aggregate_check():
    """The split-bf16 product without the lo halves of its inputs is a bf16 product: the aggregate check must catch it on every
    case, whatever the per-element bound does."""
    for c, layout in SMALL:
        if layout == "bf16x3":
            worst = {}
            run(c, layout, ("split_lo_dropped_in",), worst, enforce=False)
            assert worst["rms"] > 2 * gm.RATIO["bf16x3"], (c["name"], worst)


def test_room_between_ratio_and_the_smallest_mistake():
    """(c) the smallest aggregate ratio a value mistake produces, per layout, and the mistake that comes closest to passing."""
    closest = {}
    for mistake in gm.MISTAKES:
        if mistake in STORES:
            continue
        for c, layout in SMALL:
            if not APPLIES[mistake](c, layout):
                continue
            worst = {}
            run(c, layout, (mistake,), worst, enforce=False)
            if layout not in closest or worst["rms"] < closest[layout][0]:
                closest[layout] = (worst["rms"], mistake, c["name"])
    for layout, (ratio, mistake, name) in sorted(closest.items()):
        print(f"{layout}: the mistake closest to passing the aggregate check is {mistake} on {name}, ratio {ratio:.2f} "
              f"(RATIO {gm.RATIO[layout]})")
        assert ratio > gm.RATIO[layout], (layout, mistake, name, ratio)
    assert set(closest) == set(gm.LAYOUTS)
