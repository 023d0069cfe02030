"""Independent restatement of DESIGN 1.6 - count(T and within(r_min:r_max, R)) - in numpy.

It imports neither the package nor the oracle.  Every atom of T and R is wrapped first (SPEC S2 per periodic axis; S3t for a tilted
cell; an open axis keeps the raw coordinate), the pair displacement is SPEC S3 (image by comparison with half the edge) or S3t (image by
rounding in fractional space), d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) and d = sqrtf(d2), all in exact fp32 (the round-to-odd fmaf of
tests/geometry_ref.py).  A target atom is in iff SOME reference atom - itself included - has r_min <= d < r_max (closed: d <= r_max).
All pairs, no cells.  `slab` is the one shortcut, for the 33 334 x 33 334 sets of the full-size test: on a periodic, untilted x axis a
reference atom whose wrapped x is further than r_max (+ 1e-3) from the target's, around the seam, cannot be in range whatever y and z
are - |dx| <= d -, so such pairs are dropped before the arithmetic; every pair that is kept is computed exactly as above.

count64() is a float64 minimum-image count by rounding: used only to show how rarely the two differ (ties at the interval ends)."""
import numpy as np

from geometry_ref import Box, fmaf

f32 = np.float32


def wrap(xyz, box):
    """xyz float32 [3, n] -> the wrapped positions float32 [3, n] the pair computation sees"""
    x, y, z = (np.asarray(v, np.float32) for v in xyz)
    if box.tri:
        Lx, Ly, Lz = box.L
        iLx, iLy, iLz = box.iL
        sz = z * iLz
        sy = fmaf(-box.yz, sz, y) * iLy
        sx = fmaf(-box.xz, sz, fmaf(-box.xy, sy, x)) * iLx
        out = []
        for s in (sx, sy, sz):
            s = s - np.floor(s)
            out.append(np.where(s < f32(1.0), s, f32(0.0)).astype(np.float32))
        sx, sy, sz = out
        ux, uy, uz = sx * Lx, sy * Ly, sz * Lz
        return np.stack([fmaf(box.xz, sz, fmaf(box.xy, sy, ux)), fmaf(box.yz, sz, uy), uz])
    out = []
    for k, v in enumerate((x, y, z)):
        if not box.p[k]:
            out.append(v)
            continue
        L, iL = box.L[k], box.iL[k]
        w = fmaf(-np.floor(v * iL), L, v)
        w = np.where(w < 0, w + L, w).astype(np.float32)
        w = np.where(w >= L, w - L, w).astype(np.float32)
        out.append(w)
    return np.stack(out)


def pair_d(box, t, r):
    """t float32 [3, nt, 1], r float32 [3, 1, nr] (wrapped) -> d float32 [nt, nr]"""
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
        d = [d0[0] - shx, d0[1] - shy, d0[2] - shz]
    else:
        d = []
        for k in range(3):
            v = d0[k]
            if box.p[k]:
                L = box.L[k]
                h = f32(0.5) * L
                v = v - np.where(v > h, L, np.where(v < -h, -L, f32(0.0))).astype(np.float32)
            d.append(v)
    d2 = fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0]))
    return np.sqrt(d2.astype(np.float32))


def hits(xyz, box, target, ref, rmin, rmax, closed=False, slab=False, chunk=512):
    """one frame: bool [len(target)] - which target atoms have a reference atom in range"""
    rmin, rmax = f32(rmin), f32(rmax)
    target, ref = np.asarray(target, np.int64), np.asarray(ref, np.int64)
    t = wrap(xyz[:, target], box)
    r = wrap(xyz[:, ref], box)
    slab = slab and not box.tri and box.p[0]
    if slab:
        order = np.argsort(r[0], kind="stable")
        r = r[:, order]
        rx = r[0].astype(np.float64)
        Lx, reach = float(box.L[0]), float(rmax) + 1.0e-3
        torder = np.argsort(t[0], kind="stable")          # a chunk of x-neighbours keeps a narrow slab
        t = t[:, torder]
    out = np.zeros(target.size, bool)
    for a in range(0, target.size, chunk):
        tc = t[:, a:a + chunk]
        rr = r
        if slab:
            lo, hi = float(tc[0].min()) - reach, float(tc[0].max()) + reach
            keep = np.zeros(r.shape[1], bool)
            for s in (-Lx, 0.0, Lx):
                keep[np.searchsorted(rx, lo + s, "left"):np.searchsorted(rx, hi + s, "right")] = True
            rr = r[:, keep]
        if rr.shape[1] == 0:
            continue
        d = pair_d(box, tc[:, :, None], rr[:, None, :])
        ok = (d >= rmin) & ((d <= rmax) if closed else (d < rmax))
        out[a:a + chunk] = ok.any(axis=1)
    if slab:
        unsorted = np.zeros_like(out)
        unsorted[torder] = out
        out = unsorted
    return out


def counts(coords, box, target, ref, rmin, rmax, closed=False, exclude_ref=False, flags=7, frames=None, slab=False):
    """coords float32 [F, 3, N] -> float32 [len(frames)]: the property's rows.  exclude_ref: T minus R (D-WITHIN-SELF flipped)"""
    target = np.asarray(target, np.int64)
    if exclude_ref:
        target = target[~np.isin(target, np.asarray(ref, np.int64))]
    frames = range(coords.shape[0]) if frames is None else frames
    if target.size == 0:
        return np.zeros(len(frames), np.float32)
    out = []
    for f in frames:
        bx = Box(box[f] if isinstance(box, list) else box, flags)
        out.append(hits(coords[f], bx, target, ref, rmin, rmax, closed, slab).sum())
    return np.asarray(out, np.float32)


def count64(xyz, box, target, ref, rmin, rmax, closed=False, chunk=512):
    """float64, minimum image by rounding on the raw coordinates: the textbook count"""
    x = np.asarray(xyz, np.float64)
    t, r = x[:, np.asarray(target, np.int64)], x[:, np.asarray(ref, np.int64)]
    n = 0
    for a in range(0, t.shape[1], chunk):
        d = box.mi_f64(*(t[k, a:a + chunk, None] - r[k, None, :] for k in range(3)))
        dd = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        ok = (dd >= float(rmin)) & ((dd <= float(rmax)) if closed else (dd < float(rmax)))
        n += int(ok.any(axis=1).sum())
    return n
