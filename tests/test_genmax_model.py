"""The float64 model, the bounds and the checks of genmax_model.py on the CPU: the numpy emulation of the kernel's scheme passes
every check of every launch test_gpu_genmax.py makes; each of a list of deliberate mistakes is caught, by a named check; the
undecided-row cap holds for the model alone; and cn_genmax_pack (host only) gives the fragment layouts the model states."""
import ctypes as C

import numpy as np
import pytest

import genmax_model as gx
from cassnat_asr_public_amd import hip

PAIRS = [(c, layout) for c in gx.CASES for layout in c["layouts"]]


def launches_of(c, layout):
    return [(kind, mode) for cc, ll, kind, mode in gx.LAUNCHES if cc is c and ll == layout]


@pytest.fixture(scope="module", autouse=True)
def forget_models():
    yield
    gx._MODEL.clear()
    gx._RAW.clear()


@pytest.mark.parametrize("c, layout", PAIRS, ids=[f"{c['name']}@{layout}" for c, layout in PAIRS])
def test_the_emulation_passes_every_check_and_the_model_alone_decides_its_rows(c, layout):
    for kind, mode in launches_of(c, layout):
        before = gx.buffers(c, layout, kind, mode)
        after = gx.emulate_launch(c, layout, kind, before)
        seen = {}
        gx.check_launch(c, layout, kind, before, after, seen)
        # the emulation's exponentials and logarithm are correctly rounded: the derived part alone must cover it
        assert seen["fast"] <= 0.0, (kind, mode, seen)
        # the cap on undecided rows, from the model alone
        res = gx.model_of(c, layout, before)
        undecided = float((~res["decided"]).mean())
        assert undecided <= (0.0 if c["data"] in gx.PLANTED else gx.UNDECIDED_CAP), (c["name"], layout, undecided)


def test_the_planted_cases_plant_what_they_claim():
    for layout in ("bf16", "bf16x3"):
        kernel = gx.LAYOUTS[layout][3]
        c = gx.BY_NAME[("dups-V1028", layout)]
        v, dup = gx.winner_of(c, layout)
        assert len(set(v) | set(dup)) == 2 * c["M"] and dup[-1] == c["V"] - 1
        assert {int(d) for d in (dup - v)[:-1]} == set(gx.dup_deltas(kernel, c["V"]))
        res = gx.model_of(c, layout, gx.buffers(c, layout, "lse", None))
        assert (res["arg"] == v).all() and res["decided"].all()
        h, W, b, dup_of = gx.raw(c, layout)
        assert (W[dup] == W[v]).all() and (b[dup] == b[v]).all() and (dup_of[dup] == v).all()
    for name, layout in (("wins-V384", "bf16"), ("wins-V1028", "fp16"), ("wins-V257", "bf16x3")):
        c = gx.BY_NAME[(name, layout)]
        res = gx.model_of(c, layout, gx.buffers(c, layout, "lse", None))
        assert sorted(res["arg"]) == list(range(c["V"])) and res["decided"].all()      # every entry wins one row
    c = gx.BY_NAME[("peaked-V1028", "bf16")]
    res = gx.model_of(c, "bf16", gx.buffers(c, "bf16", "lse", None))
    top2 = np.sort(res["l"], -1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0] > 36).all() and (res["maxlp"] > -1e-12).all()
    c = gx.BY_NAME[("flat-V384", "bf16")]
    res = gx.model_of(c, "bf16", gx.buffers(c, "bf16", "lse", None))
    assert (res["arg"] == 0).all() and np.allclose(res["maxlp"], -np.log(384), atol=1e-12)
    # V = 384: wave 3 of the 16-bit kernel holds nothing but padding, and the odd tile count was rounded up
    assert gx.vtw_of("16", 384) == 4 and 32 * 3 * 4 >= 384 and gx.vtw_of("16", 40) == 2 and gx.vtw_of("16", 6144) == 48
    assert gx.vtw_of("split", 6144) == 24 and gx.vtw_of("split", 1) == 1


# mistake: (case, layout, kind, target mode, the check that must catch it)
CAUGHT_BY = {
    "map_r": ("wins-V384", "bf16", "argmax", None, "argmax-decided"),
    "half_offset_dropped": ("wins-V384", "fp16", "argmax", None, "argmax-decided"),
    "tie_high_fold": ("dups-V1028", "bf16", "argmax", None, "argmax-tie"),
    "tie_high_half": ("dups-V1028", "bf16x3", "argmax", None, "argmax-tie"),
    "tie_high_wave": ("dups-V1028", "fp16", "lse", None, "argmax-tie"),
    "no_rescale": ("shape-M97-V1028", "bf16", "lse", None, "maxlp-bound"),
    "wave_merge_no_rescale": ("shape-M65-V1028", "bf16x3", "lse", None, "maxlp-bound"),
    "pad_bias_zero": ("shape-M33-V40", "bf16", "lse", None, "maxlp-bound"),
    "last_tile_dropped": ("wins-V257", "bf16x3", "argmax", None, "argmax-decided"),
    "no_bias": ("halfneg-V1028", "bf16", "lse", None, "argmax-decided"),
    "maxlp_is_max_logit": ("shape-M33-V384", "fp16", "lse", None, "maxlp-bound"),
    "gather_returns_logit": ("shape-M33-V384", "bf16", "gather", "mixed", "tgt-bound"),
    "gather_ld_as_u": ("shape-M63-V384", "bf16", "gather", "mixed", "untouched"),
    "m_dev_ignored": ("mdev-70-of-96", "bf16", "lse", None, "untouched"),
    "split_no_wlo_xhi": ("shape-M65-V1028", "bf16x3", "lse", None, "maxlp-bound"),
    "split_no_whi_xlo": ("shape-M65-V1028", "bf16x3", "gather", "mixed", "tgt-bound"),
    "half_pack_as_bf16": ("shape-M97-V1028", "fp16", "gather", "mixed", "tgt-bound"),
}
_CAUGHT = {}


def caught(mistake):
    """(check, ratio or None, text) of the LaunchError the mistake raises in its row of CAUGHT_BY."""
    if mistake not in _CAUGHT:
        name, layout, kind, mode, _ = CAUGHT_BY[mistake]
        c = gx.BY_NAME[(name, layout)]
        before = gx.buffers(c, layout, kind, mode)
        gx.check_launch(c, layout, kind, before, gx.emulate_launch(c, layout, kind, before))  # (right, it passes)
        with pytest.raises(gx.LaunchError) as e:
            gx.check_launch(c, layout, kind, before, gx.emulate_launch(c, layout, kind, before, (mistake,)))
        _CAUGHT[mistake] = (e.value.check, e.value.ratio, str(e.value))
    return _CAUGHT[mistake]


def test_every_listed_mistake_has_a_row():
    assert set(CAUGHT_BY) == set(gx.MISTAKES)


@pytest.mark.parametrize("mistake", gx.MISTAKES)
def test_each_mistake_is_caught_by_the_named_check(mistake):
    check, ratio, text = caught(mistake)
    print(f"{mistake}: caught by {check}" + (f" at {ratio:.3g} x the bound" if ratio else "") + f"  ({text})")
    assert check == CAUGHT_BY[mistake][4], text


def test_the_closest_mistake_per_bound_check_is_well_outside():
    """The mistake that misses a bound by the least still misses it by a factor."""
    closest = {}
    for mistake in gx.MISTAKES:
        check, ratio, _ = caught(mistake)
        if ratio:
            closest[check] = min(closest.get(check, (np.inf, "")), (ratio, mistake))
    assert set(closest) == {"maxlp-bound", "tgt-bound"}
    for check, (ratio, mistake) in sorted(closest.items()):
        print(f"closest to passing {check}: {mistake} at {ratio:.3g} x the bound")
        assert ratio > 2.0, (check, mistake, ratio)


def test_the_tie_mistakes_are_each_seen_only_by_their_own_distance():
    """A tie to the higher index in the fold shows between entries of one lane (next entry, next tile), in the half merge at distance
    4, in the wave merge one wave away: the planted distances are all needed."""
    c = gx.BY_NAME[("dups-V1028", "bf16")]
    before = gx.buffers(c, "bf16", "argmax", None)
    v, dup = gx.winner_of(c, "bf16")
    deltas = gx.dup_deltas("16", c["V"])
    want = {"tie_high_fold": {deltas[0], deltas[2]}, "tie_high_half": {deltas[1]}, "tie_high_wave": {deltas[3]}}
    for mistake, dist in want.items():
        after = gx.emulate_launch(c, "bf16", "argmax", before, (mistake,))
        got = after["arg"][gx.GUARD:gx.GUARD + c["M"]]
        hit = {int(d) for d in (dup - v)[:-1][got[:-1] != v[:-1]]}
        assert hit == dist, (mistake, hit)


@pytest.mark.parametrize("layout", list(gx.LAYOUTS))
@pytest.mark.parametrize("V", [1, 40, 384, 1028, 6144])
def test_the_pack_is_the_layout_the_model_states(layout, V):
    flavour, prec, operand, kernel = gx.LAYOUTS[layout]
    L = hip.lib(flavour)
    assert L.cn_operand16().decode() == operand
    rng = np.random.default_rng(V)
    W = (rng.standard_normal((V, gx.D)) / 16).astype(np.float32)
    W[0, :4] = [1e-3, -3.0, 0.0, 65000.0]  # (small, large and a value half precision barely holds)
    b = rng.standard_normal(V).astype(np.float32)
    want_w, want_b = gx.pack_model(W, b, V, layout)
    got_w, got_b = np.full(want_w.size, 0xABCD, np.uint16), np.full(want_b.size, 7.0, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.cn_genmax_pack(prec, ptr(W), ptr(b), V, ptr(got_w), got_w.nbytes, ptr(got_b), got_b.size)
    assert rc == 0, L.cn_last_error()
    assert want_w.size == gx.WAVES[kernel] * gx.vtw_of(kernel, V) * 16 * (1024 if kernel == "split" else 512)
    assert np.array_equal(got_w, want_w.reshape(-1))
    assert np.array_equal(got_b.view(np.uint32), want_b.view(np.uint32))
    # padded vocabulary rows are zero, padded biases -inf - stated once more without the model's index arithmetic
    frag = got_w.reshape(gx.WAVES[kernel] * gx.vtw_of(kernel, V), -1, 64, 8)  # [tile][ks (x plane)][lane][j]
    entry = 32 * np.arange(frag.shape[0])[:, None] + (np.arange(64) & 31)[None, :]
    assert (frag[np.broadcast_to((entry >= V)[:, None, :, None], frag.shape)] == 0).all()
    assert np.isneginf(got_b[V:]).all() and np.array_equal(got_b[:V], b)
    # the other library's build of the same sources does not own this precision; sizes are checked
    other = hip.lib("f16" if flavour is None else None)
    assert other.cn_genmax_pack(prec, ptr(W), ptr(b), V, ptr(got_w), got_w.nbytes, ptr(got_b), got_b.size) == -1
    assert other.cn_last_error().decode().startswith("cn_genmax_pack: ")
    assert L.cn_genmax_pack(prec, ptr(W), ptr(b), V, ptr(got_w), got_w.nbytes - 2, ptr(got_b), got_b.size) == -1
    assert L.cn_last_error().decode().startswith("cn_genmax_pack: ")
