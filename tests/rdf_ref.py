"""Independent restatement of SPEC S4 - the integer histogram of rdf(ref, target, r_min:r_max) - in numpy and Python integers.

It imports neither the package nor the oracle.  Two tiers.

fp32 tier (the contract).  Positions are wrapped and pair distances formed by tests/within_ref.py (wrap, pair_d: SPEC S2 / S3 / S3t in
exact fp32 with the round-to-odd fmaf of tests/geometry_ref.py).  S4 follows in np.float32 with one rounding per operation:

    w = fl(r_max - r_min);  inv_range = fl(1 / w);  a = fl(d - r_min);  p = fl(a * inv_range);  t = fl(p * 1024);  bin = (int)t, clamped

hit iff r_min < d < r_max (closed: r_min <= d <= r_max).  All ordered pairs, i == j included, u64 counts.  The counts of a frame depend
only on the multiset of its pair distances, so `distances` forms it once and `histogram` bins it for any number of ranges.
`distances` has one shortcut: a plain float32 estimate of the minimum-image distance (`_estimate`, good to 2e-5 for coordinates below 64) sorts out the pairs farther
than keep_below + 1e-4 before the exact arithmetic; every pair that is kept is computed exactly as above.  Where the estimate takes
another image than S3 / S3t does - a component within rounding of half a cell - the pair is kept or dropped by chance, and is out of
range either way as long as keep_below + 2e-4 stays below half the smallest cell width (asserted).

Exact tier (the mathematics).  The same fp32 d, r_min, r_max taken as the rationals they are:

    t* = 1024 (d - r_min) / (r_max - r_min),   bin* = floor(t*), clamped

in integer arithmetic on the values scaled by 2^40 (every fp32 value of magnitude in [2^-17, 2^23) is an integer then, and
1024 (d - r_min) 2^40 < 2^63; anything smaller goes through fractions.Fraction).  No fp64, no tolerance.

The margin (`margin`).  With u = 2^-24 and |e_i| <= u:
    a = (d - r_min)(1 + e1)                                       the subtraction (exact where Sterbenz applies; bounded anyway)
    p = a inv_range (1 + e2)                                      the first product
    t = 1024 p                                                    the second product: 1024 = 2^10, exact (no overflow, no subnormal here)
    inv_range = rho / (r_max - r_min)                             rho is a constant of the range: `rho` computes it exactly, as a Fraction
so t = t* rho (1 + e1)(1 + e2), and
    |t - t*| <= t* (|rho - 1| + rho (2 u + u^2)) =: margin(t*).
rho itself carries the two roundings of inv_range, |rho - 1| <= 2 u + u^2, so margin(t*) <= t* (4 u + 5 u^2) < 2.5e-7 t* whatever the
range; with t* <= 1024 (a hit has d <= r_max) the margin stays below 2.5e-4 bins.  As margin < 1/2:
    |bin - bin*| <= 1, and bin != bin* only where t* lies within margin(t*) of an integer
(truncation is monotone; the clamp to [0, 1023] is applied to both and cannot widen a difference).  `compare` asserts both statements
pair by pair and reports how many pairs differ and the worst offset as a fraction of its margin."""
from fractions import Fraction

import numpy as np

from geometry_ref import Box
import within_ref as W

f32 = np.float32
NBINS = 1024
U = 2.0 ** -24
SCALE = 40                      # fp32 values are held as integers in units of 2^-40


def distances(xyz, box, ref, tgt, keep_below, chunk=256):
    """one frame: the fp32 distances of all ordered pairs (i in ref, j in tgt) with d <= keep_below, float32 [n], unordered.
    xyz float32 [3, N]; box a geometry_ref.Box"""
    ref, tgt = np.asarray(ref, np.int64), np.asarray(tgt, np.int64)
    r = W.wrap(np.asarray(xyz, np.float32)[:, ref], box)
    t = W.wrap(np.asarray(xyz, np.float32)[:, tgt], box)
    assert float(keep_below) + 2.0e-4 < 0.5 * _width(box), "the estimate's image is only safe below half the cell"
    out = []
    for a in range(0, ref.size, chunk):
        ii, jj = np.nonzero(_estimate(box, r[:, a:a + chunk, None], t[:, None, :]) <= f32(keep_below + 1.0e-4))
        d = W.pair_d(box, r[:, a + ii], t[:, jj])
        out.append(d[d <= f32(keep_below)])
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def _width(box):
    """the smallest distance between opposite periodic faces (inf: no periodic axis)"""
    if not any(box.p):
        return np.inf
    A = np.array([[box.L[0], box.xy, box.xz], [0.0, box.L[1], box.yz], [0.0, 0.0, box.L[2]]], np.float64)
    w = 1.0 / np.linalg.norm(np.linalg.inv(A), axis=1)
    return float(min(w[k] for k in range(3) if box.p[k]))


def _estimate(box, a, b):
    """plain float32 minimum-image distance of wrapped positions (broadcasting [3, ...] arrays): a filter, never a result"""
    d = [a[k] - b[k] for k in range(3)]
    if box.tri:
        n = np.rint(d[2] / box.L[2]); d[2] = d[2] - n * box.L[2]; d[1] = d[1] - n * box.yz; d[0] = d[0] - n * box.xz
        n = np.rint(d[1] / box.L[1]); d[1] = d[1] - n * box.L[1]; d[0] = d[0] - n * box.xy
        d[0] = d[0] - np.rint(d[0] / box.L[0]) * box.L[0]
    else:
        for k in range(3):
            if box.p[k]:
                d[k] = d[k] - np.rint(d[k] / box.L[k]) * box.L[k]
    return np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


def d_of(box, a, b):
    """the fp32 distance of the positions a[:, k] and b[:, k] (float32 [3, n], as stored): the same arithmetic, pair by pair"""
    return W.pair_d(box, W.wrap(np.asarray(a, np.float32), box), W.wrap(np.asarray(b, np.float32), box))


def pair_distance(xyz, box, i, j):
    """the fp32 distance of the atom pairs (i[k], j[k]), float32 [len(i)]"""
    x = np.asarray(xyz, np.float32)
    return d_of(box, x[:, np.asarray(i, np.int64)], x[:, np.asarray(j, np.int64)])


def bins32(d, rmin, rmax, closed=False):
    """S4 in fp32: int64 [n], -1 where the pair is no hit"""
    d, rmin, rmax = np.asarray(d, np.float32), f32(rmin), f32(rmax)
    inv_range = f32(1.0) / f32(rmax - rmin)
    hit = ((rmin <= d) & (d <= rmax)) if closed else ((rmin < d) & (d < rmax))
    a = (d - rmin).astype(np.float32)
    p = (a * inv_range).astype(np.float32)
    t = (p * f32(NBINS)).astype(np.float32)
    b = np.clip(np.trunc(np.where(hit, t, f32(0.0))).astype(np.int64), 0, NBINS - 1)
    return np.where(hit, b, -1)


def histogram(d, rmin, rmax, closed=False):
    """u64 [1024] of the distances d"""
    b = bins32(d, rmin, rmax, closed)
    return np.bincount(b[b >= 0], minlength=NBINS).astype(np.uint64)


def counts(coords, box, ref, tgt, rmin, rmax, closed=False, flags=7, frames=None):
    """coords float32 [F, 3, N] -> u64 [1024] summed over the frames"""
    out = np.zeros(NBINS, np.uint64)
    for f in (range(coords.shape[0]) if frames is None else frames):
        bx = Box(box[f] if isinstance(box, list) else box, flags)
        out += histogram(distances(coords[f], bx, ref, tgt, rmax), rmin, rmax, closed)
    return out


# ---- the exact tier ---------------------------------------------------------------------------------------------------------------------

def _scaled(v):
    """fp32 -> the integer v 2^40, int64; asserts that it is one"""
    x = np.asarray(v, np.float32).astype(np.float64) * 2.0 ** SCALE          # a power of two: exact
    assert np.all(x == np.rint(x)) and np.all(np.abs(x) < 2.0 ** 52), "not an integer at 2^-40"
    return x.astype(np.int64)


def rho(rmin, rmax):
    """inv_range (r_max - r_min), exactly"""
    rmin, rmax = f32(rmin), f32(rmax)
    inv_range = f32(1.0) / f32(rmax - rmin)
    return Fraction(float(inv_range)) * (Fraction(float(rmax)) - Fraction(float(rmin)))


def margin(tstar, rmin, rmax):
    """the derived bound of |t - t*| at the exact scaled position(s) tstar (float64 is ample for a bound)"""
    r = rho(rmin, rmax)
    return np.abs(tstar) * (float(abs(r - 1)) + float(r) * (2.0 * U + U * U))


def exact(d, rmin, rmax, closed=False):
    """-> (bin* int64 [n] with -1 for no hit, num int64 [n], den int): t* = num / den for the hits, floor and remainder in integers"""
    d, rmin, rmax = np.asarray(d, np.float32), f32(rmin), f32(rmax)
    hit = ((rmin <= d) & (d <= rmax)) if closed else ((rmin < d) & (d < rmax))
    Rmin, Rmax = int(_scaled(rmin)), int(_scaled(rmax))
    den = Rmax - Rmin
    assert den > 0
    x = d.astype(np.float64) * 2.0 ** SCALE
    fine = x == np.rint(x)
    num = np.zeros(d.shape, np.int64)
    ok = hit & fine
    num[ok] = (x[ok].astype(np.int64) - Rmin) * NBINS
    assert np.all(num[ok] >= 0) and (Rmax - Rmin) * NBINS < 2 ** 62
    b = np.where(ok, np.minimum(num // den, NBINS - 1), -1)
    for k in np.nonzero(hit & ~fine)[0]:                                      # distances below 2^-17: Fractions
        t = (Fraction(float(d[k])) - Fraction(float(rmin))) * NBINS / (Fraction(float(rmax)) - Fraction(float(rmin)))
        b[k] = min(t.numerator // t.denominator, NBINS - 1)
        num[k] = -1                                                           # not on the integer grid: see compare()
    return b, num, den


def compare(d, rmin, rmax, closed=False, what=""):
    """the two statements of the module's head, asserted for every distance of d.  -> dict(differ, near, worst): pairs whose bins differ,
    pairs with t* within its margin of an integer, worst |offset| / margin among the pairs that differ"""
    d = np.asarray(d, np.float32)
    b32 = bins32(d, rmin, rmax, closed)
    bx, num, den = exact(d, rmin, rmax, closed)
    assert np.array_equal(b32 < 0, bx < 0), f"{what}: the tiers disagree about the interval"
    hit = bx >= 0
    grid = hit & (num >= 0)
    diff = np.abs(b32 - bx)
    assert diff[hit].max(initial=0) <= 1, f"{what}: the fp32 bin is {diff[hit].max()} bins from the exact one"
    rem = np.where(grid, num % den, 0)
    off = np.minimum(rem, den - rem)                                          # |t* - nearest integer| den, an integer
    tstar = np.where(grid, num.astype(np.float64) / den, 0.0)
    m = margin(tstar, rmin, rmax)
    near = grid & (off.astype(np.float64) <= m * den)
    differ = hit & (diff != 0)
    assert not (differ & ~grid).any(), f"{what}: a distance below 2^-17 changes bin"
    bad = differ & ~near
    assert not bad.any(), (f"{what}: {int(bad.sum())} pairs change bin outside the margin, e.g. d = {d[bad][0]!r}, t* = {tstar[bad][0]!r}, "
                           f"margin {m[bad][0]:.3g}")
    worst = float((off[differ] / (m[differ] * den)).max()) if differ.any() else 0.0
    return dict(differ=int(differ.sum()), near=int(near.sum()), worst=worst, hits=int(hit.sum()))


def offsets(d, rmin, rmax):
    """|t* - nearest integer| of every distance as float64 (a figure for reports: the parked pairs of the device's fast path)"""
    d = np.asarray(d, np.float32)
    t = (d.astype(np.float64) - float(f32(rmin))) * NBINS / (float(f32(rmax)) - float(f32(rmin)))
    return np.abs(t - np.rint(t))


def fast_delta(rmin, rmax):
    """the budget of the device's fast path (vmd_make_binning), restated in fp32: delta = 2.5e-4 + 6e-7 T, T = r_max inv_range nbins.
    The fast path is used at all iff delta < 0.25."""
    rmin, rmax = f32(rmin), f32(rmax)
    inv_range = f32(1.0) / f32(rmax - rmin)
    return f32(f32(2.5e-4) + f32(f32(f32(f32(6.0e-7) * rmax) * inv_range) * f32(NBINS)))
