"""Independent restatement of DESIGN S6b (angle / dihedral) in numpy + the standard library.

It imports neither the package nor the oracle: every step is written out from the contract text.  Argument points are the S6 centres
of distance(a, b) (mass-weighted, fp64 sums in index order, de-periodised sequentially against the set's first atom, rounded to fp32);
the difference vectors are fp32 minimum images by rounding (orthorhombic per axis, triclinic in fractional space); the value is formed in
fp64 without fused operations, with math.atan2, and rounded once to fp32.  Vectorised over contexts: within a context the atoms are
still summed one after the other in their index-list order, exactly as the device does.
"""
import math

import numpy as np

f32 = np.float32
DEG = 180.0 / math.pi


def fmaf(a, b, c):
    """fp32 fused multiply-add, correctly rounded: the fp64 product of two fp32 values is exact; the fp64 sum is made exact with
    TwoSum and rounded to odd before the single rounding to fp32 (53 >= 24 + 2 bits, so no double-rounding error)."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64)
    even = (bits & 1) == 0
    fix = (e != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


class Box:
    """One frame's cell as the kernels see it: L, fl(1/L), tilts, periodic axes, triclinic flag.  box: None (open), scalar (cube),
    (x, y, z) or (x, y, z, xy, xz, yz); flags: the unit cell's periodic-axis bits (7 = all)."""

    def __init__(self, box, flags=7):
        if box is None:
            box, flags = (0.0, 0.0, 0.0), 0
        if np.isscalar(box):
            box = (box, box, box)
        box = tuple(box) + (0.0,) * (6 - len(box))
        self.L = [f32(v) for v in box[:3]]
        self.iL = [f32(1.0) / v if v > 0 else f32(np.inf) for v in self.L]
        self.xy, self.xz, self.yz = (f32(v) for v in box[3:6])
        self.p = [bool(flags & (1 << k)) and self.L[k] > 0 for k in range(3)]
        self.tri = self.xy != 0 or self.xz != 0 or self.yz != 0

    def mi_f64(self, dx, dy, dz):
        """S6 de-periodisation in fp64: d - L rint(d / L) per periodic axis; triclinic: rint in fractional space"""
        if self.tri:
            Lx, Ly, Lz = (float(v) for v in self.L)
            xy, xz, yz = float(self.xy), float(self.xz), float(self.yz)
            sz = dz / Lz
            sy = (dy - yz * sz) / Ly
            sx = (dx - xy * sy - xz * sz) / Lx
            sx = sx - np.rint(sx); sy = sy - np.rint(sy); sz = sz - np.rint(sz)
            return sx * Lx + xy * sy + xz * sz, sy * Ly + yz * sz, sz * Lz
        out = []
        for k, d in enumerate((dx, dy, dz)):
            L = float(self.L[k])
            out.append(d - L * np.rint(d / L) if self.p[k] else d)
        return tuple(out)

    def mi_f32(self, dx, dy, dz):
        """the fp32 minimum image of a difference vector (S6: fmaf(-rintf(d * invL), L, d); triclinic: S3t frac / cart)"""
        dx, dy, dz = (np.asarray(v, np.float32) for v in (dx, dy, dz))
        if self.tri:
            Lx, Ly, Lz = self.L
            iLx, iLy, iLz = self.iL
            sz = dz * iLz
            sy = fmaf(-self.yz, sz, dy) * iLy
            sx = fmaf(-self.xz, sz, fmaf(-self.xy, sy, dx)) * iLx
            sx = sx - np.rint(sx); sy = sy - np.rint(sy); sz = sz - np.rint(sz)
            return fmaf(self.xz, sz, fmaf(self.xy, sy, sx * Lx)), fmaf(self.yz, sz, sy * Ly), sz * Lz
        out = []
        for k, d in enumerate((dx, dy, dz)):
            out.append(fmaf(-np.rint(d * self.iL[k]), self.L[k], d) if self.p[k] else d)
        return tuple(out)


def set_centres(xyz, box, sets, mass):
    """S6 centre of every context's set: xyz float32 [3, N]; sets: list of P index arrays; mass float32 [N] -> float32 [3, P]"""
    P = len(sets)
    n = np.array([len(s) for s in sets])
    assert P and n.min() > 0, "empty set"
    width = n.max()
    idx = np.zeros((P, width), np.int64)
    for c, s in enumerate(sets):
        idx[c, :len(s)] = s
    x = [xyz[k].astype(np.float64) for k in range(3)]
    w_all = np.asarray(mass, np.float32).astype(np.float64)
    sw = np.zeros(P)
    sx, sy, sz = np.zeros(P), np.zeros(P), np.zeros(P)
    p0 = [x[k][idx[:, 0]] for k in range(3)]
    for a in range(width):
        live = a < n
        i = idx[:, a]
        q = [x[k][i] for k in range(3)]
        if a > 0:
            d = box.mi_f64(q[0] - p0[0], q[1] - p0[1], q[2] - p0[2])
            q = [p0[k] + d[k] for k in range(3)]
        w = w_all[i]
        sw = np.where(live, sw + w, sw)
        sx = np.where(live, sx + w * q[0], sx)
        sy = np.where(live, sy + w * q[1], sy)
        sz = np.where(live, sz + w * q[2], sz)
    return np.stack([sx / sw, sy / sw, sz / sw]).astype(np.float32)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _atan2(y, x):
    # `+ 0.0`: a -0 operand becomes +0 (D-ANGLE-DEGENERATE: atan2(0, 0) = 0; no dihedral of -180)
    return np.array([math.atan2(float(a) + 0.0, float(b) + 0.0) for a, b in zip(y, x)], np.float64)


def frame_values(xyz, box, arg_sets, mass, radians=False):
    """one frame: arg_sets = 3 (angle) or 4 (dihedral) lists of P index arrays -> float32 [P]"""
    pts = [set_centres(xyz, box, s, mass) for s in arg_sets]

    def diff(i, j):     # fp32 mi(p_i - p_j), promoted to fp64
        d = box.mi_f32(pts[i][0] - pts[j][0], pts[i][1] - pts[j][1], pts[i][2] - pts[j][2])
        return tuple(np.asarray(v, np.float32).astype(np.float64) for v in d)

    if len(arg_sets) == 3:
        u, v = diff(0, 1), diff(2, 1)
        cr = _cross(u, v)
        rad = _atan2(np.sqrt(_dot(cr, cr)), _dot(u, v))
    else:
        b1, b2, b3 = diff(1, 0), diff(2, 1), diff(3, 2)
        n1, n2 = _cross(b1, b2), _cross(b2, b3)
        rad = _atan2(np.sqrt(_dot(b2, b2)) * _dot(b1, n2), _dot(n1, n2))
    return (rad if radians else rad * DEG).astype(np.float32)


def values(coords, box, arg_sets, mass=None, radians=False, geometric=False, flags=7, frames=None):
    """coords float32 [F, 3, N]; box as Box() takes it, or a list of one per frame; arg_sets: per argument a list of P index arrays (a
    single index array = one context).  mass None or geometric=True: unit weights (D-DIST-COM).  -> float32 [len(frames), P]"""
    F, _, N = coords.shape
    arg_sets = [[np.asarray(s, np.int64).reshape(-1)] if np.ndim(s[0]) == 0 else [np.asarray(x, np.int64).reshape(-1) for x in s]
                for s in arg_sets]
    m = np.ones(N, np.float32) if (mass is None or geometric) else np.asarray(mass, np.float32)
    frames = range(F) if frames is None else frames
    out = []
    for f in frames:
        bx = Box(box[f] if isinstance(box, list) else box, flags)
        out.append(frame_values(coords[f], bx, arg_sets, m, radians))
    return np.stack(out)
