"""The checks of ffn_model.py would catch what the fused feed-forward kernels can get wrong - shown on the CPU, on the case list the
GPU test (test_gpu_ffn.py) runs.  A launch is stood in for by chain_model's EMULATION writing the launch's buffers: alone it passes
every case in both layouts; with one deliberate mistake it fails at least one case, and the table (-s) names the check that
catches it.  As in test_chain_model.py, the 0.2 % LayerNorm mistakes (biased std) must be caught in the fp16 layout; in the bf16
layout they are as large as the operand's own roundoff and their ratios are printed, not required."""
import pytest

import chain_model as cm
import ffn_model as fm

FOUND = {}
APPLIES = {
    "ln1_biased_std": lambda c: True,
    "lnn_biased_std": lambda c: c["has_next"],
    "ln1_eps_in_var": lambda c: c["adv"],
    "lnn_eps_in_var": lambda c: c["has_next"] and c["adv"] and c["tiny_w2"],
    "no_b1": lambda c: True,
    "no_b2": lambda c: True,
    "no_residual_ffn": lambda c: True,
    "act_swapped": lambda c: True,
    "slice_dropped": lambda c: c["nslice"] > 1,
    "slice_twice": lambda c: c["nslice"] > 1,
    "slice_shifted": lambda c: c["nslice"] > 1,
    "lnn_from_old_x": lambda c: c["has_next"],
    "rows_past_m_stored": lambda c: True,
}
SMALL = ("ln1_biased_std", "lnn_biased_std")


def run(c, layout, mistakes=(), worst=None, enforce=True):
    before = fm.buffers(c, layout)
    after = {k: v.clone() for k, v in before.items()}
    fm.emulate_launch(c, layout, after, mistakes)
    fm.check_launch(c, layout, before, after, worst, enforce)


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    print("\nmistake: what catches it first per layout (check, case, rms ratio of an aggregate failure)")
    for (name, layout), (kind, case, ratio) in sorted(FOUND.items()):
        print(f"  {name:20s} {layout:5s} {kind:10s} {case:44s} {'' if ratio is None else f'{ratio:.1f}'}")
    fm._MODEL.clear()


def test_case_list_covers_what_the_issue_names():
    assert set(APPLIES) == set(fm.MISTAKES)
    names = [c["name"] for c in fm.CASES]
    assert len(set(names)) == len(names)
    whole = [c for c in fm.CASES if c["nslice"] == 1]
    for swish in (False, True):
        for has_next in (False, True):
            assert {c["M"] for c in whole if c["swish"] == swish and c["has_next"] == has_next} >= set(fm.M_ALL)
    assert {c["dff"] for c in fm.CASES} == {128, 256, 1024, 2048} and {c["nslice"] for c in fm.CASES} == {1, 2, 4, 8, 16}
    assert all(c["dff"] % (128 * c["nslice"]) == 0 for c in fm.CASES)
    for dff, ns in ((2048, 8), (1024, 4)):  # run_ffn_step's launches, both activations, with the next LayerNorm
        for swish in (False, True):
            assert any(c["dff"] == dff and c["nslice"] == ns and c["swish"] == swish and c["has_next"] for c in fm.CASES)
    assert any(c["nslice"] > 1 and not c["has_next"] for c in fm.CASES)
    assert any(c["nslice"] == 1 and not c["has_next"] and not c["swish"] and c["M"] <= 32 for c in fm.CASES)  # MT = 1, ReLU, no norm


@pytest.mark.parametrize("layout", fm.LIBS)
def test_the_emulation_alone_passes_every_case(layout):
    for c in fm.CASES:
        worst = {}
        run(c, layout, worst=worst)
        assert all(r <= 1.0 + 1e-9 for _, r in worst.values()), (c["name"], worst)


@pytest.mark.parametrize("mistake", fm.MISTAKES)
def test_mistake_is_caught(mistake):
    cases = [c for c in fm.CASES if APPLIES[mistake](c)]
    assert cases, "no case of the GPU test can show this mistake"
    caught = {}
    for layout in fm.LIBS:
        for c in cases:
            try:
                run(c, layout, (mistake,))
            except fm.LaunchError as e:
                caught[layout] = FOUND[(mistake, layout)] = (e.kind, c["name"], e.ratio)
                break
    assert "fp16" in caught, f"{mistake}: no case catches it in the fp16 layout"
    if mistake not in SMALL:
        assert "bf16" in caught, f"{mistake}: no case catches it in the bf16 layout"
    if mistake == "rows_past_m_stored":
        assert all(kind == "untouched" for kind, _, _ in caught.values())


@pytest.mark.parametrize("layout", fm.LIBS)
def test_room_between_ratio_and_the_smallest_mistake(layout):
    """The smallest aggregate ratio each mistake produces over the cases it applies to; RATIO must sit below every one of them in
    the fp16 layout (bf16: below all but the two 0.2 % LayerNorm mistakes, whose figures are printed)."""
    closest = None
    for mistake in fm.MISTAKES:
        if mistake == "rows_past_m_stored":
            continue
        ratios = []
        for c in [c for c in fm.CASES if APPLIES[mistake](c)][:10]:
            worst = {}
            try:
                run(c, layout, (mistake,), worst, enforce=False)
            except fm.LaunchError:  # not finite
                continue
            ratios.append((max(r for _, r in worst.values()), c["name"]))
        low = min(ratios)
        print(f"{layout} {mistake}: smallest rms ratio {low[0]:.2f} ({low[1]}), largest {max(ratios)[0]:.2f}")
        if layout == "fp16" or mistake not in SMALL:
            assert low[0] > fm.RATIO[layout], (mistake, low)
            if closest is None or low[0] < closest[0]:
                closest = (low[0], mistake, low[1])
    print(f"{layout}: the mistake closest to passing the aggregate check is {closest[1]} on {closest[2]}, ratio {closest[0]:.2f} "
          f"(RATIO {fm.RATIO[layout]})")
