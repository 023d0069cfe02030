"""Independent restatement of DESIGN 1.15 - solvent-accessible surface area by Shrake-Rupley - in numpy.

It imports neither the package nor the oracle.  All pairs, no cells, fp32 operation by operation (the wrap and the round-to-odd fmaf of
tests/within_ref.py, the image of tests/hbond_ref.py).  R = radius + probe, one fp32 add per list entry; r_cut = 2 max(R) over both lists.
Environment entry j - through its canonical entry, D-SASA-COINCIDENT: entries whose wrapped coordinates coincide bit for bit answer as the
lowest of them, with its atom and its R - is a neighbour of measured entry i iff
  1. distance: both wrapped (SPEC S2 / S3t), e = (i - j) - shift with the SPEC S3 / S3t image, d2 = fmaf(ez, ez, fmaf(ey, ey, ex ex)),
     d = sqrtf(d2), 0 <= d < r_cut (closed: <= r_cut);
  2. d2 < s * s strictly, s = R_i + R_j;
  3. j's atom is not i's atom, by index.
Point k of entry i is buried by neighbour j iff (u_kx * e_x + u_ky * e_y) + u_kz * e_z < t_ij, t_ij = ((R_j * R_j - R_i * R_i) - d2) /
(R_i + R_i), every operation rounded on its own; n_i = the points no neighbour buries.  w_i = llround(4 pi R_i^2 / P * 2^20) in double, the
frame's total the integer sum of n_i w_i, the temporal value float32(float64(total) * 2^-20).
The points u_k are an ARGUMENT (the library's table, vmd_sasa_points): libm's last bit is nobody's contract.  points_formula() is the numpy
statement of D-SASA-POINTS the table is held to within 1 ulp.
near: how many candidate pairs (rule 1 passed) lie within 4 ulp of s * s, and how many point tests within 4 ulp of t_ij."""
import math

import numpy as np

from hbond_ref import boxes_of, canonical, delta, ulps_between
from within_ref import fmaf, wrap

f32 = np.float32


def points_formula(P):
    """D-SASA-POINTS in float64, rounded once -> float32 [P, 3]"""
    k = np.arange(P, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / P
    rho = np.sqrt(1.0 - z * z)
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1).astype(np.float32)


def big_r(radius, probe):
    return (np.asarray(radius, np.float32) + f32(probe)).astype(np.float32)


def r_cut_of(R_meas, R_env):
    m = max(f32(R_meas.max()), f32(R_env.max()))
    return f32(m + m)


def weights(R, P):
    """w_i = llround(4 pi R_i^2 / P * 2^20), python ints"""
    return [int(math.floor(4.0 * math.pi * float(r) * float(r) / P * 1048576.0 + 0.5)) for r in R]


def frame_counts(xyz, box, meas, R_meas, env, R_env, points, r_cut, closed=False, chunk=128):
    """one frame -> (n uint32 [nmeas], neighbours (how many (i, j) pass all three rules), near_s, near_t)"""
    meas, env = np.asarray(meas, np.int64), np.asarray(env, np.int64)
    P = len(points)
    ux, uy, uz = (np.ascontiguousarray(points[:, k], np.float32)[:, None] for k in range(3))
    mw = wrap(xyz[:, meas], box)
    ew = wrap(xyz[:, env], box)
    canon = canonical(ew)
    atom_j = env[canon]
    Rj = np.asarray(R_env, np.float32)[canon]
    Rj2 = (Rj * Rj).astype(np.float32)
    out = np.zeros(meas.size, np.uint32)
    neighbours = near_s = near_t = 0
    for a in range(0, meas.size, chunk):
        sl = slice(a, a + chunk)
        Ri = np.asarray(R_meas, np.float32)[sl]
        e = delta(box, mw[:, sl, None], ew[:, None, :])
        d2 = fmaf(e[2], e[2], fmaf(e[1], e[1], e[0] * e[0])).astype(np.float32)
        d = np.sqrt(d2)
        hit = (d <= r_cut) if closed else (d < r_cut)
        s = (Ri[:, None] + Rj[None, :]).astype(np.float32)
        s2 = (s * s).astype(np.float32)
        near_s += int((hit & (ulps_between(d2, s2) <= 4)).sum())
        nb = hit & (d2 < s2) & (atom_j[None, :] != meas[sl, None])
        Ri2 = (Ri * Ri).astype(np.float32)
        t = (((Rj2[None, :] - Ri2[:, None]).astype(np.float32) - d2).astype(np.float32) / (Ri + Ri).astype(np.float32)[:, None]).astype(np.float32)
        for i in range(Ri.size):
            idx = np.nonzero(nb[i])[0]
            neighbours += idx.size
            if not idx.size:
                out[a + i] = P
                continue
            ex, ey, ez = (np.asarray(e[k], np.float32)[i, idx][None, :] for k in range(3))
            dot = ((ux * ex).astype(np.float32) + (uy * ey).astype(np.float32)).astype(np.float32)
            dot = (dot + (uz * ez).astype(np.float32)).astype(np.float32)
            tt = t[i, idx][None, :]
            near_t += int((ulps_between(dot, np.broadcast_to(tt, dot.shape)) <= 4).sum())
            out[a + i] = P - int((dot < tt).any(axis=1).sum())
    return out, neighbours, near_s, near_t


def evaluate(coords, box, meas, meas_radius, env, env_radius, probe, points, closed=False, flags=7, frames=None):
    """coords float32 [F, 3, N]; frames: the evaluated frames in order, a frame named twice counts twice.
    -> dict(area float32 [F] (0 where not evaluated), record uint64 [nmeas + 1], counts {frame: uint32 [nmeas]}, totals {frame: int},
            neighbours, near_s, near_t)"""
    F = coords.shape[0]
    frames = list(range(F)) if frames is None else list(frames)
    meas, env = np.asarray(meas, np.int64), np.asarray(env, np.int64)
    R_meas, R_env = big_r(meas_radius, probe), big_r(env_radius, probe)
    r_cut = r_cut_of(R_meas, R_env)
    P = len(points)
    w = weights(R_meas, P)
    rec = np.zeros(meas.size + 1, np.uint64)
    area = np.zeros(F, np.float32)
    counts, totals = {}, {}
    neighbours = near_s = near_t = 0
    for f in frames:
        if f not in counts:
            n, nn, ns, nt = frame_counts(coords[f], boxes_of(box, flags, f), meas, R_meas, env, R_env, points, r_cut, closed)
            counts[f] = n
            totals[f] = sum(int(c) * wi for c, wi in zip(n, w))
            neighbours += nn
            near_s += ns
            near_t += nt
        area[f] = f32(np.float64(totals[f]) * 2.0 ** -20)
        rec[:-1] += counts[f].astype(np.uint64)
        rec[-1] += np.uint64(1)
    return dict(area=area, record=rec, counts=counts, totals=totals, neighbours=neighbours, near_s=near_s, near_t=near_t)
