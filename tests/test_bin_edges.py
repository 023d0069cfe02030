"""tests/rdf_ref.py judged on the CPU, on every system of tests/bin_edge_cases.py: the coverage conditions, the exact tier with its margin
(rdf_ref.compare, inside coverage()), and the fp32 tier against the oracle's all-pairs evaluation bit for bit - which gives the oracle an
independent judge as well.  Run with -s for the figures."""
import numpy as np
import pytest

import bin_edge_cases as B
import rdf_ref as R


@pytest.mark.parametrize("rname", list(B.RANGES))
@pytest.mark.parametrize("cell", B.CELLS)
def test_coverage_and_exact_tier(cell, rname):
    B.coverage(B.system(cell, rname))


@pytest.mark.parametrize("rname", list(B.RANGES))
@pytest.mark.parametrize("cell", B.CELLS)
def test_fp32_tier_is_the_oracle(oracle, cell, rname):
    B.against_oracle(oracle, B.system(cell, rname))


def test_fast_path_thresholds():
    """vmd_make_binning's delta = 2.5e-4 + 6e-7 T, T = r_max inv_range 1024, on which side of 0.25 each range falls, and the width at
    which r_max = 12 leaves the fast path"""
    for name, (rmin, rmax, fast) in B.RANGES.items():
        assert (float(R.fast_delta(rmin, rmax)) < 0.25) == fast, name
    assert abs(float(R.fast_delta(11.9, 12.0)) - 0.074) < 1.0e-3
    width = 6.0e-7 * 12.0 * 1024 / (0.25 - 2.5e-4)                     # 0.02952
    assert 12.0 - 11.97 > width > 12.0 - 11.971
    assert float(R.fast_delta(12.0 - 1.001 * width, 12.0)) < 0.25 <= float(R.fast_delta(12.0 - 0.999 * width, 12.0))


def test_exact_tier_on_every_float_around_every_edge():
    """every float within 3 of every edge: the fp32 bin is the exact one or its neighbour, and differs only inside the margin"""
    for name, (rmin, rmax, _) in B.RANGES.items():
        e = B.edges(rmin, rmax)
        d = np.unique(np.concatenate([B.step(e, k) for k in range(-3, 4)]))
        d = d[d > 0]
        c = R.compare(d, rmin, rmax, closed=True, what=name)
        print(f"rdf_ref {name}: {d.size} floats within 3 of an edge, {c['near']} within the margin, {c['differ']} with another bin in fp32 "
              f"(worst offset {c['worst']:.3f} of its margin)")


def test_tiers_on_small_distances():
    """below 2^-17 the exact tier goes through Fractions: the bins of bin 0 and of a range that starts below them"""
    d = np.float32([2.0 ** -30, 3.0e-8, 2.0 ** -18, 1.0e-5])
    c = R.compare(d, 0.0, 3.2, what="small")
    assert c["hits"] == 4 and c["differ"] == 0
    np.testing.assert_array_equal(R.bins32(d, 0.0, 2.0 ** -16), np.trunc(d.astype(np.float64) * 2.0 ** 26).astype(np.int64))
