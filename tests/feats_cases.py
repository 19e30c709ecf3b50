"""One list of cases for the matrix compression (tests/feats_model.py): the model tests, the host-twin tests and the kernel tests all
walk it.  A case is a padded float32 batch (rows, Tmax, F) and its int32 lengths; rows at or behind a length are NaN unless the case
says otherwise, so that anything that reads them shows."""
import numpy as np

import feats_model as M

f32 = np.float32
TS = (1, 8, 9, 10, 12, 13, 63, 64, 65, 257, 1031)
FS = (1, 3, 16, 17, 80, 83, 240)


def _batch(mats, tmax=None, pad=np.nan):
    tmax = tmax or max(m.shape[0] for m in mats)
    out = np.full((len(mats), tmax, mats[0].shape[1]), pad, f32)
    for r, m in enumerate(mats):
        out[r, :m.shape[0]] = m
    return out, np.array([m.shape[0] for m in mats], np.int32)


def _case(name, mats, **kw):
    lens = kw.pop("lens", None)
    feats, own = _batch([np.asarray(m, f32) for m in mats], **kw)
    return {"name": name, "feats": feats, "lens": own if lens is None else np.asarray(lens, np.int32)}


def code_grid(rng, T, F, R=37.5):
    """A matrix all of whose values are dequantised codes of the range [0, R]: a column's values at its quartile indices then ARE its
    P25 / P75 as the reader computes them, so the comparisons `v < P25` / `v < P75` meet equality."""
    inc = f32(R) * M.U16_INC
    x = (inc * rng.randint(1, 65000, size=(T, F)).astype(f32)).astype(f32)
    x[0, 0], x[1, 0] = 0.0, R
    return x


def make_cases():
    rng = np.random.RandomState(20240607)
    cases = []
    for T in TS:
        for F in FS:
            cases.append(_case("gauss_T%d_F%d" % (T, F), [rng.randn(T, F) * 3 - 1]))
    for rows, F in ((1, 80), (3, 83), (33, 17)):
        lens = [int(n) for n in rng.choice([1, 2, 7, 8, 9, 10, 17, 64, 65, 100], size=rows)]
        lens[0] = 9
        if rows > 1:
            lens[1], lens[-1] = 8, 70
        cases.append(_case("ragged_%d" % rows, [rng.randn(n, F) * (1 + r % 3) for r, n in enumerate(lens)], tmax=max(lens) + 3))
    for T, F in ((10, 3), (64, 17), (257, 16)):
        cases.append(_case("ties_T%d_F%d" % (T, F), [np.round(rng.randn(T, F) * 2) / 4]))
    cases.append(_case("constant", [np.full((12, 3), 2.5), np.full((5, 3), -7.0), np.zeros((9, 3)), np.full((9, 3), -0.0)]))
    x = rng.randn(40, 5)
    x[:, 2] = 0.25
    cases.append(_case("constant_column", [x]))
    x = rng.randn(33, 4)
    x[:, 1] = x.max()
    x[:, 3] = x.min()
    cases.append(_case("column_at_the_extremes", [x]))
    x = rng.randn(65, 6) * np.array([1e-6, 1.0, 1e4, 1e-3, 30.0, 1e-6]) + np.array([-5.0, 0.0, -2e4, 7.0, -100.0, 9e3])
    cases.append(_case("tiny_beside_huge", [x]))
    cases.append(_case("on_the_quartiles", [code_grid(rng, 16, 3), code_grid(rng, 65, 3), code_grid(rng, 9, 3)]))
    # at a minimum of 512 a uint16 step (range / 65535 = 1.5e-5) is a quarter of a float32 ulp (6.1e-5): the forced-apart header codes of
    # a constant column dequantise to ONE float, P0 == P25 == the value - the only place where `<=` for `<` at P25 changes a byte
    # (0 / 0 in the first segment instead of the start of the next)
    x = 512 + rng.rand(12, 3)
    x[:, 1] = 512.4
    x[0, 0], x[1, 0] = 512.0, 513.0
    cases.append(_case("constant_column_below_an_ulp", [x]))
    cases.append(_case("lens_above_tmax", [rng.randn(20, 5), rng.randn(20, 5), rng.randn(6, 5)], lens=[25, 20, 2 ** 30], pad=0.5))
    x = [rng.randn(12, 4), rng.randn(12, 4), rng.randn(5, 4), rng.randn(12, 4), rng.randn(3, 4)]
    x[1][7, 2] = np.nan
    x[2][0, 0] = np.inf
    x[3][11, 3] = -np.inf
    cases.append(_case("not_finite", x))
    cases.append(_case("no_rows", [rng.randn(10, 4), rng.randn(10, 4), rng.randn(10, 4)], lens=[0, 10, -3]))
    return cases


CASES = make_cases()


def valid(case, r):
    """Utterance r's valid rows (the lengths are clamped to the batch)."""
    return case["feats"][r, :max(0, min(int(case["lens"][r]), case["feats"].shape[1]))]
