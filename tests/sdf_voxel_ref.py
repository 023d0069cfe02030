"""Independent restatement of SPEC S5's scatter - target atom -> voxel of structure k's volume - in numpy and Python rationals.

It imports neither the package nor the oracle.  R32, c32 are inputs here (the alignment has tests/sdf_align_ref.py).  Two tiers.

fp32 tier (the contract), one rounding per step, fmaf by the round-to-odd construction of tests/geometry_ref.py:

    d  = fl(p - c32) per axis;  image: d = fmaf(-rintf(fl(d invL)), L, d) per periodic axis (a triclinic cell: S3t's frac / rint / cart)
    qx = fmaf(R02, dz, fmaf(R01, dy, fl(R00 dx)))        (qy, qz alike)
    vscale = fl(dim / fl(2 s));  a = fl(q + s);  t = fl(a vscale)
    in iff 0 <= t < dim on all three axes;  v = (int)t;  vol[(vz dim + vy) dim + vx] += 1

`0 <= t` lets t = -0.0 into voxel 0 (in_range, voxel).  No input produces it: q + s with s > 0 is +0 or at least half a float of s away
from 0, and the product with vscale >= 1 does not underflow.  A target atom that is a member of structure k is skipped for k
(D-SDF-EXCL) unless include_self.

Exact tier.  d - the fp32 displacement after the image step - R32 and s taken as the rationals they are:

    q* = R d (exact),   t* = (q* + s) dim / (2 s),   v* = floor(t*)

The margin (`exact` returns it with t*).  u = 2^-24, |e_i| <= u:
    q  = q* + eq,  |eq| <= g3 B,  B = |R0 dx| + |R1 dy| + |R2 dz|,  g3 = 3 u / (1 - 3 u)       (a product and two fused steps)
    a  = (q + s)(1 + e4);   t = a vscale (1 + e5);   vscale = rho dim / (2 s), rho exact (`rho`), |rho - 1| <= 2 u + u^2
so  t = (t* + eq dim / (2 s)) rho (1 + e4)(1 + e5)  and with w = rho (1 + u)^2
    |t - t*| <= g3 B dim / (2 s) w + |t*| (|rho - 1| + rho (2 u + u^2)) =: margin.
margin < 1/2, hence |v - v*| <= 1 and v != v* only where t* lies within its margin of an integer; a target is in for one tier and out
for the other only where t* lies within its margin of 0 or dim.  `compare` asserts this axis by axis."""
from fractions import Fraction

import numpy as np

from geometry_ref import fmaf

f32 = np.float32
U = 2.0 ** -24


def vscale_of(s, dim=128):
    return f32(f32(dim) / f32(f32(2.0) * f32(s)))


def displacement(p, box, c):
    """p float32 [3, n], c float32 [3] -> the fp32 image displacement d [3, n] (box: a geometry_ref.Box)"""
    d = [(np.asarray(p[k], np.float32) - f32(c[k])).astype(np.float32) for k in range(3)]
    return np.stack([np.asarray(v, np.float32) for v in box.mi_f32(*d)])


def t_of(p, box, R, c, s, dim=128):
    """-> (t float32 [3, n], d float32 [3, n])"""
    R = np.asarray(R, np.float32).reshape(3, 3)
    d = displacement(p, box, c)
    vs = vscale_of(s, dim)
    t = []
    for r in range(3):
        q = fmaf(R[r, 2], d[2], fmaf(R[r, 1], d[1], (R[r, 0] * d[0]).astype(np.float32)))
        a = (q + f32(s)).astype(np.float32)
        t.append((a * vs).astype(np.float32))
    return np.stack(t), d


def in_range(t, dim=128):
    t = np.asarray(t, np.float32)
    return ((t >= f32(0.0)) & (t < f32(dim))).all(axis=0)


def voxel(t):
    """(int)t per axis (call for targets in range only): -0.0 -> 0"""
    return np.trunc(np.asarray(t, np.float32)).astype(np.int64)


def scatter(xyz, box, R32, c32, tgt, s, dim=128, structs=None, include_self=False, vol=None):
    """one frame: xyz float32 [3, N]; R32 [K, 3, 3], c32 [K, 3]; tgt atom indices; structs [K, m] or None -> u64 [dim^3] (added to vol)"""
    vol = np.zeros(dim ** 3, np.uint64) if vol is None else vol
    tgt = np.asarray(tgt, np.int64)
    p = np.asarray(xyz, np.float32)[:, tgt]
    for k in range(len(R32)):
        t, _ = t_of(p, box, R32[k], c32[k], s, dim)
        ok = in_range(t, dim)
        if structs is not None and not include_self:
            ok &= ~np.isin(tgt, np.asarray(structs[k], np.int64))
        v = voxel(t[:, ok])
        np.add.at(vol, (v[2] * dim + v[1]) * dim + v[0], np.uint64(1))
    return vol


# ---- the exact tier ---------------------------------------------------------------------------------------------------------------------

def rho(s, dim=128):
    """vscale 2 s / dim, exactly"""
    return Fraction(float(vscale_of(s, dim))) * 2 * Fraction(float(f32(s))) / dim


def exact(d, R, s, dim=128):
    """d float32 [3, n] -> (t* as Fractions [3][n], margin float64 [3, n])"""
    R = np.asarray(R, np.float32).reshape(3, 3)
    S, r = Fraction(float(f32(s))), rho(s, dim)
    g3 = 3.0 * U / (1.0 - 3.0 * U)
    w = float(r) * (1.0 + U) ** 2
    dr = float(abs(r - 1)) + float(r) * (2.0 * U + U * U)
    n = d.shape[1]
    ts, m = [[None] * n for _ in range(3)], np.zeros((3, n))
    D = [[Fraction(float(d[j, i])) for i in range(n)] for j in range(3)]
    for a in range(3):
        Ra = [Fraction(float(R[a, j])) for j in range(3)]
        for i in range(n):
            terms = [Ra[j] * D[j][i] for j in range(3)]
            t = (sum(terms) + S) * dim / (2 * S)
            ts[a][i] = t
            m[a, i] = g3 * float(sum(abs(x) for x in terms)) * dim / (2.0 * float(S)) * w + abs(float(t)) * dr
    return ts, m


def compare(p, box, R, c, s, dim=128, what=""):
    """the statements of the module's head for the targets p float32 [3, n]; -> dict(differ, near, flips, worst)"""
    t, d = t_of(p, box, R, c, s, dim)
    ts, m = exact(d, R, s, dim)
    assert m.max(initial=0.0) < 0.5
    differ = near = flips = 0
    worst = 0.0
    for a in range(3):
        for i in range(t.shape[1]):
            tx, t32 = ts[a][i], float(t[a, i])
            off = abs(tx - round(tx))
            is_near = float(off) <= m[a, i]
            near += is_near
            in32, inx = 0.0 <= t32 < dim, 0 <= tx < dim
            if in32 != inx:
                flips += 1
                assert min(abs(float(tx)), abs(float(tx) - dim)) <= m[a, i], f"{what}: axis {a}, target {i}: in for one tier, out for the other at t* = {float(tx)!r}"
            if in32 and inx:
                v32, vx = int(np.trunc(t32)), tx.numerator // tx.denominator
                assert abs(v32 - vx) <= 1, f"{what}: axis {a}, target {i}: voxel {v32} against {vx}"
                if v32 != vx:
                    differ += 1
                    assert is_near, f"{what}: axis {a}, target {i}: voxel {v32} against {vx} at t* = {float(tx)!r}, margin {m[a, i]:.3g}"
                    worst = max(worst, float(off) / m[a, i])
    return dict(differ=differ, near=int(near), flips=flips, worst=worst, n=3 * t.shape[1])
