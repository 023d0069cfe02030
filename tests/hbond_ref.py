"""Independent restatement of DESIGN 1.14 - hydrogen bonds between a donor set and an acceptor set - in numpy.

It imports neither the package nor the oracle.  All pairs, no cells, fp32 operation by operation (the wrap and the round-to-odd fmaf of
tests/within_ref.py / tests/geometry_ref.py).  A bond is one (donor pair j, acceptor entry k) combination with
  1. distance: D and A wrapped (SPEC S2 / S3t), e = (D - A) - shift with the SPEC S3 / S3t image, d2 = fmaf(ez, ez, fmaf(ey, ey, ex ex)),
     d = sqrtf(d2), 0 <= d < r_da (closed: <= r_da);
  2. identity: the acceptor's atom is neither the pair's donor nor its hydrogen, by atom index;
  3. hydrogen: h = the fp32 minimum image by rounding of (H - D) from the RAW frame (distance()'s image);
  4. angle: u = -h, v = -e - h, uu = (ux ux + uy uy) + uz uz and so on, every operation rounded on its own:
     uu > 0 and vv > 0 and dot <= 0 and dot * dot >= c2 * (uu * vv), c2 = fl32(cos^2(angle_min)) formed in double (90 and 180 degrees: 0 and
     1 exactly).
D-HB-COINCIDENT: acceptor entries whose wrapped coordinates coincide bit for bit in a frame all answer as the lowest such entry - for the
identity test, the acceptor row and the pair list alike.
near(): how many candidate pairs lie within 4 ulp of the distance threshold, and how many distance hits within 4 ulp of the angle's."""
import math

import numpy as np

from geometry_ref import Box
from within_ref import fmaf, wrap

f32 = np.float32


def c2_of(angle_min_deg):
    a = float(f32(angle_min_deg))
    cs = 0.0 if a == 90.0 else -1.0 if a == 180.0 else math.cos(a * (math.pi / 180.0))
    return f32(cs * cs)


def delta(box, t, r):
    """wrapped t float32 [3, nt, 1], r float32 [3, 1, nr] -> e = (t - r) - shift, three float32 [nt, nr]"""
    d0 = [np.asarray(t[k] - r[k], np.float32) for k in range(3)]
    if box.tri:
        Lx, Ly, Lz = box.L
        iLx, iLy, iLz = box.iL
        sz = d0[2] * iLz
        sy = fmaf(-box.yz, sz, d0[1]) * iLy
        sx = fmaf(-box.xz, sz, fmaf(-box.xy, sy, d0[0])) * iLx
        nx, ny, nz = np.rint(sx), np.rint(sy), np.rint(sz)
        shx = fmaf(nz, box.xz, fmaf(ny, box.xy, nx * Lx))
        shy = fmaf(nz, box.yz, ny * Ly)
        shz = nz * Lz
        return [d0[0] - shx, d0[1] - shy, d0[2] - shz]
    d = []
    for k in range(3):
        v = d0[k]
        if box.p[k]:
            L = box.L[k]
            h = f32(0.5) * L
            v = v - np.where(v > h, L, np.where(v < -h, -L, f32(0.0))).astype(np.float32)
        d.append(v)
    return d


def dot3(a, b):
    return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]).astype(np.float32)


def canonical(aw):
    """aw float32 [3, nacc] wrapped -> int64 [nacc]: the lowest entry with the same three bit patterns"""
    keys = np.ascontiguousarray(aw.T).view(np.int32).reshape(-1, 3)
    first = {}
    out = np.zeros(len(keys), np.int64)
    for k, key in enumerate(map(tuple, keys)):
        out[k] = first.setdefault(key, k)
    return out


def ulps_between(a, b):
    def line(v):
        i = np.asarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(line(a) - line(b))


def frame_bonds(xyz, box, donor, hydrogen, acceptor, r_da, angle_min_deg, closed=False, chunk=256):
    """one frame -> (pairs int64 [n, 2] = {pair j, canonical acceptor entry} in ascending (j, list position) order, near_d, near_a)"""
    donor, hydrogen, acceptor = (np.asarray(v, np.int64) for v in (donor, hydrogen, acceptor))
    r_da, c2 = f32(r_da), c2_of(angle_min_deg)
    dw = wrap(xyz[:, donor], box)
    aw = wrap(xyz[:, acceptor], box)
    canon = canonical(aw)
    a_atom = acceptor[canon]
    h = box.mi_f32(*(xyz[k][hydrogen] - xyz[k][donor] for k in range(3)))
    out = []
    near_d = near_a = 0
    for a in range(0, donor.size, chunk):
        sl = slice(a, a + chunk)
        e = delta(box, dw[:, sl, None], aw[:, None, :])
        d2 = fmaf(e[2], e[2], fmaf(e[1], e[1], e[0] * e[0]))
        d = np.sqrt(d2.astype(np.float32))
        hit = (d <= r_da) if closed else (d < r_da)
        near_d += int((ulps_between(d, r_da) <= 4).sum())
        hh = [np.asarray(v, np.float32)[sl, None] for v in h]
        u = [-v for v in hh]
        v = [(-e[k] - hh[k]).astype(np.float32) for k in range(3)]
        uu = dot3(u, u) + np.zeros_like(d)
        vv = dot3(v, v)
        dot = dot3(u, v)
        lhs = (dot * dot).astype(np.float32)
        rhs = (c2 * (uu * vv).astype(np.float32)).astype(np.float32)
        near_a += int((hit & (dot <= 0) & (ulps_between(lhs, rhs) <= 4)).sum())
        other = (a_atom[None, :] != donor[sl, None]) & (a_atom[None, :] != hydrogen[sl, None])
        ok = hit & other & (uu > 0) & (vv > 0) & (dot <= 0) & (lhs >= rhs)
        jj, kk = np.nonzero(ok)            # row-major: ascending (pair, list position)
        out.append(np.stack([jj + a, canon[kk]], axis=1))
    pairs = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    return pairs, near_d, near_a


def boxes_of(box, flags, f):
    return Box(box[f] if isinstance(box, list) else box, flags)


def evaluate(coords, box, donor, hydrogen, acceptor, r_da, angle_min_deg, closed=False, flags=7, frames=None):
    """coords float32 [F, 3, N]; frames: the evaluated frames in order, a frame named twice counts twice.
    -> dict(counts float32 [F] (0 where not evaluated), record uint64 [npairs + nacc + 1], pairs {frame: int32 [n, 3] atom triples},
            near_d, near_a)"""
    F = coords.shape[0]
    frames = list(range(F)) if frames is None else list(frames)
    donor, hydrogen, acceptor = (np.asarray(v, np.int64) for v in (donor, hydrogen, acceptor))
    npairs, nacc = donor.size, acceptor.size
    rec = np.zeros(npairs + nacc + 1, np.uint64)
    counts = np.zeros(F, np.float32)
    triples = {}
    near_d = near_a = 0
    for f in frames:
        pairs, nd, na = frame_bonds(coords[f], boxes_of(box, flags, f), donor, hydrogen, acceptor, r_da, angle_min_deg, closed)
        near_d += nd
        near_a += na
        counts[f] = f32(len(pairs))
        rec[:npairs] += np.bincount(pairs[:, 0], minlength=npairs).astype(np.uint64)
        rec[npairs:npairs + nacc] += np.bincount(pairs[:, 1], minlength=nacc).astype(np.uint64)
        rec[-1] += np.uint64(1)
        triples[f] = np.stack([donor[pairs[:, 0]], hydrogen[pairs[:, 0]], acceptor[pairs[:, 1]]], axis=1).astype(np.int32)
    return dict(counts=counts, record=rec, pairs=triples, near_d=near_d, near_a=near_a)
