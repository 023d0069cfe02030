"""a10 pinned to the reference ITSELF: compute_histogram, compute_histogram_masked, downsample_histogram and scale_histogram are
plain C++ inside the reference's src/main.cpp:139-261.  oracle/make_ref.py cuts those line ranges out of the reference's sources
and compiles them (oracle/_ref/libviamd_ref.so, git-ignored); tests/golden/make_ref_pin.py runs that compiled reference code
on the inputs below and stores what it returned in tests/golden/ref_pin.npz.  Here the oracle's restatement (vo_*) and the
product's host functions (vmd_*) are held against those stored outputs on random and adversarial inputs - bit for bit, NaNs
included - and, where the compiled reference can be built, the stored outputs against the reference code itself.  This is the
formula the 1e-5 tolerance of normalised g(r) is measured through."""
import ctypes as C
import os
from collections import Counter

import numpy as np
import pytest

import viamd_amd as V
from viamd_amd import eval as E

from oracle import make_ref

fp, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pin.npz")


def load_ref_lib():
    """the compiled reference (oracle/_ref/libviamd_ref.so), or None where neither the reference's sources nor a prebuilt library is present"""
    path = make_ref.build()
    if path is None:
        return None
    lib = C.CDLL(path)
    lib.ref_compute_histogram.argtypes = [fp, C.c_int, C.c_float, C.c_float, fp, C.c_int, fp, fp]
    lib.ref_compute_histogram_masked.argtypes = [fp, C.c_int, C.c_float, C.c_float, fp, C.c_int, u8p, C.c_int, C.c_int, fp]
    lib.ref_downsample_histogram.argtypes = [fp, C.c_int, fp, fp, C.c_int]
    lib.ref_scale_histogram.argtypes = [fp, fp, C.c_int]
    for f in (lib.ref_compute_histogram, lib.ref_compute_histogram_masked, lib.ref_downsample_histogram, lib.ref_scale_histogram):
        f.restype = None
    return lib


class Ref:
    """The reference's histogram functions as the test `test` calls them: each call returns the output stored for it in
    tests/golden/ref_pin.npz (the n-th call of a kind within that test), checked bit for bit against the compiled reference when `lib`
    is there.  record: a dict that receives the compiled reference's outputs instead (tests/golden/make_ref_pin.py)."""

    def __init__(self, test, lib, golden, record=None):
        self.test, self.lib, self.golden, self.record = test, lib, golden, record
        self.calls = Counter()

    def _want(self, kind, run):
        key = f"{self.test}.{kind}_{self.calls[kind]}"
        self.calls[kind] += 1
        if self.record is not None:
            self.record[key] = run()
            return self.record[key]
        want = self.golden[key]
        if self.lib is not None:
            assert same(run(), want), ("stored output differs from the compiled reference", key)
        return want

    def compute_histogram(self, nb, lo, hi, values):
        """-> (bins, min, max)"""
        def run():
            want = np.zeros(nb, np.float32)
            mn, mx = C.c_float(-1), C.c_float(-1)
            self.lib.ref_compute_histogram(_f(want), nb, lo, hi, _f(values), values.size, C.byref(mn), C.byref(mx))
            return np.append(want, np.float32([mn.value, mx.value]))
        r = self._want("compute_histogram", run)
        return r[:nb], r[nb], r[nb + 1]

    def compute_histogram_masked(self, nb, lo, hi, v, dim, mask, agg):
        """-> (bins, y range); the y range starts at -7 and stays there without a frame"""
        n = (1 if agg else dim) * nb

        def run():
            want = np.zeros(n, np.float32)
            yr = np.full(2, -7.0, np.float32)
            self.lib.ref_compute_histogram_masked(_f(want), nb, lo, hi, _f(v), dim, mask.ctypes.data_as(u8p), mask.size, int(agg), _f(yr))
            return np.append(want, yr)
        r = self._want("compute_histogram_masked", run)
        return r[:n], r[n:]

    def downsample_histogram(self, n_dst, src, weights):
        def run():
            want = np.zeros(n_dst, np.float32)
            self.lib.ref_downsample_histogram(_f(want), n_dst, _f(src), _f(weights) if weights is not None else None, src.size)
            return want
        return self._want("downsample_histogram", run)

    def scale_histogram(self, src, w):
        def run():
            want = src.copy()
            self.lib.ref_scale_histogram(_f(want), _f(w), src.size)
            return want
        return self._want("scale_histogram", run)


@pytest.fixture(scope="module")
def ref_source():
    with np.load(GOLDEN) as z:
        golden = {k: z[k] for k in z.files}
    return load_ref_lib(), golden


@pytest.fixture
def ref(request, ref_source):
    return Ref(request.function.__name__, *ref_source)


def _f(a):
    return a.ctypes.data_as(fp)


def same(a, b):
    """bit-identical float arrays (NaN == NaN, -0 != +0)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _value_sets(rng):
    yield rng.normal(3.0, 1.5, 4000).astype(np.float32), 0.5, 6.0
    yield rng.uniform(-1, 1, 777).astype(np.float32), -1.0, 1.0                      # values on both range ends
    yield np.array([0.0, 1.0, 1.0, 0.25, 0.999999, 1.0000001, -1e-9], np.float32), 0.0, 1.0
    yield rng.uniform(10, 11, 50).astype(np.float32), 0.0, 1.0                       # nothing inside the range
    yield np.float32(7.5) * np.ones(30, np.float32), 7.5, 7.5                        # empty range: inv_range = inf (unmasked) / 0 (masked)
    yield (rng.integers(0, 50, 5000) / np.float32(7)).astype(np.float32), 0.0, 7.0   # many values exactly on bin edges


def test_compute_histogram_against_the_reference(ref, oracle, host_lib):
    rng = np.random.default_rng(5)
    for values, lo, hi in _value_sets(rng):
        for nb in (1, 7, 128, 1024):
            want, mn, mx = ref.compute_histogram(nb, lo, hi, values)
            got_o, omn, omx = oracle.compute_histogram(values, nb, lo, hi)
            got_p, pmn, pmx = E.compute_histogram(values, nb, lo, hi, lib=host_lib)
            assert same(got_o, want) and same(got_p, want), (lo, hi, nb)
            assert same([omn, omx], [mn, mx]) and same([pmn, pmx], [mn, mx])


def test_compute_histogram_masked_against_the_reference(ref, oracle, host_lib):
    rng = np.random.default_rng(6)
    for values, lo, hi in _value_sets(rng):
        for dim in (1, 3):
            F = values.size // dim
            v = values[:F * dim]
            for mask in (np.ones(F, np.uint8), (rng.random(F) < 0.4).astype(np.uint8), np.zeros(F, np.uint8)):
                for agg in (False, True):
                    for nb in (5, 128):
                        want, yr = ref.compute_histogram_masked(nb, lo, hi, v, dim, mask, agg)
                        got_o = oracle.compute_histogram_masked(v, dim, mask, nb, lo, hi, agg)
                        got_p, pyr = E.compute_histogram_masked_y(v, dim, mask, nb, lo, hi, agg, lib=host_lib)
                        assert same(got_o, want), ("oracle", lo, hi, dim, agg, nb)
                        assert same(got_p, want), ("product", lo, hi, dim, agg, nb)
                        if mask.any():                     # without a frame the reference leaves y_min / y_max as they were
                            assert same(pyr, yr), (pyr, yr)
                        assert same(E.compute_histogram_masked(v, dim, mask, nb, lo, hi, agg, lib=host_lib), want)


def test_downsample_and_scale_against_the_reference(ref, oracle, host_lib):
    rng = np.random.default_rng(7)
    for n_src in (1024, 1000, 128, 7):
        src = rng.integers(0, 500, n_src).astype(np.float32)
        w = rng.uniform(0, 40, n_src).astype(np.float32)
        w[rng.random(n_src) < 0.1] = 0.0                      # empty source bins: 0 / 0 and x / 0 go through as the reference has them
        for n_dst in sorted({1, 2, 7, 128, n_src // 3 or 1, n_src}):
            if n_dst > n_src:
                continue
            for weights in (w, None):
                want = ref.downsample_histogram(n_dst, src, weights)
                assert same(oracle.downsample_histogram(src, weights, n_dst), want)
                assert same(V.downsample_histogram(src, weights, n_dst, lib=host_lib), want)
        want = ref.scale_histogram(src, w)
        assert same(E.scale_histogram(src, w, lib=host_lib), want)


def test_g_of_r_of_an_evaluated_rdf_through_the_reference_downsample(ref, oracle, emu_lib):
    """End to end on the a10 formula: counts and weights of an evaluated rdf() (emulator build of the product) -> the REFERENCE's
    downsample_histogram == the product's, bit for bit, and g -> 1 for the ideal gas within the statistical error."""
    import cases
    coords = cases.water_box(oracle, 9, 3000, 40.0, 4)
    o = cases.oxygen(3000)
    ir = V.ScriptIR(emu_lib); ir.add_rdf("g", o, o, 12.0)
    ev = V.ScriptEval(4, ir)
    assert ev.frame_range(V.MolSystem(3000, unitcell=V.make_unitcell(40.0)), V.HostTrajectory(coords, V.make_unitcell(40.0)), 0, 4)
    pd = ev.property_data("g")
    vals, wts = np.array(pd.values, np.float32), np.array(pd.weights, np.float32)
    want = ref.downsample_histogram(128, vals, wts)
    got = V.downsample_histogram(vals, wts, 128, lib=emu_lib)
    assert same(got, want)
    assert abs(float(np.mean(want[64:])) - 1.0) < 0.05
