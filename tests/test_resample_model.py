"""tests/resample_model.py against itself: the phase-table form equals the direct sum over every input sample, and the output
counts equal a brute-force count of the outputs whose time lies before the end of the input.  No GPU, no library."""
from fractions import Fraction

import numpy as np
import pytest

import resample_model as rm

PAIRS = rm.PAIRS + [(16000, 16000), (32000, 16000), (12000, 16000)]


@pytest.mark.parametrize("fi,fo", rm.PAIRS)
def test_table_form_equals_the_direct_sum(fi, fo):
    """Output k of the table form is sum_j x[j] * filt(j / fi - k / fo) * win(.) / fi over ALL j.  The two differ only in how the
    time offset is formed (j / fi - i / fo after the shift by whole units, against j' / fi - k / fo): an error of a few ulps of
    the times (< 0.1 s here, 2^-56) times the slope 2 pi cutoff < 1e5 of the filter's argument - below 1e-11 relative to
    sum |terms|, taken 100 times over."""
    rng = np.random.default_rng(fi + fo)
    in_unit, out_unit, first, weights = rm.table(fi, fo)
    n = 3 * in_unit + 2 * max(len(w) for w in weights) + 5
    x = rng.integers(-32768, 32768, size=n).astype(np.float64)
    y, s = rm.resample(x, fi, fo)
    assert len(y) == rm.num_samples(fi, fo, n) > 2 * out_unit
    ks = sorted(set(list(range(0, len(y), max(1, len(y) // 97))) + [0, 1, len(y) - 2, len(y) - 1, out_unit - 1, out_unit, out_unit + 1]))
    for k in ks:
        assert abs(y[k] - rm.direct(x, fi, fo, k)) <= 1e-9 * s[k] + 1e-300, (k, y[k])
    assert (s > 0).all()


def test_tap_and_phase_counts():
    got = [(max(len(w) for w in rm.table(fi, fo)[3]), rm.table(fi, fo)[1]) for fi, fo in rm.PAIRS]
    assert got == [(13, 2), (37, 1), (34, 160), (17, 320), (13, 640), (25, 1)]


def test_equal_rates_are_the_identity():
    x = np.array([-32768, 32767, 0, 5, -7], np.float64)
    y, s = rm.resample(x, 16000, 16000)
    np.testing.assert_array_equal(y, x)
    np.testing.assert_array_equal(s, np.abs(x))
    assert rm.table(16000, 16000)[:3] == (1, 1, [0])


@pytest.mark.parametrize("fi,fo", PAIRS)
def test_output_counts_against_brute_force(fi, fo):
    """Output k exists when its time k / fo lies before the end of the input, n / fi (exact rational arithmetic)."""
    in_unit, out_unit = rm.units(fi, fo)
    ns = set(range(0, 51))
    for m in (1, 2, 3, 7):
        ns.update(range(max(0, m * in_unit - 2), m * in_unit + 3))
    for n in sorted(ns):
        brute, k = 0, 0
        while Fraction(k, fo) < Fraction(n, fi):
            brute, k = brute + 1, k + 1
        assert rm.num_samples(fi, fo, n) == brute, (fi, fo, n)
    assert rm.num_samples(fi, fo, -3) == 0


def test_pick_reads_one_interleaved_channel():
    data = np.arange(12)
    np.testing.assert_array_equal(rm.pick(data, 3, 1), [1, 4, 7, 10])
    np.testing.assert_array_equal(rm.pick(data, 1, 0), data)
