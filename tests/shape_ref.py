"""Two independent restatements of DESIGN 1.4 (shape_weights) in numpy fp64.  Neither imports the package or the oracle.

pinned: the contract as the device evaluates it - offsets by the fp64 minimum image against the set's first atom, the ten moments summed
        in the documented order (chunks of 4096 atoms, 256 threads that take every 256th atom, xor butterfly over the 64 lanes of a wave,
        the four waves, the chunks), cyclic Jacobi in the documented pair order.  The emulator must agree with it bit for bit.
plain:  np.sum moments about the first atom and np.linalg.eigvalsh.  Agreement is absolute: |got - ref| <= 2^-23 (see test_shape.py).

The cell and its fp64 minimum image are geometry_ref.Box (the S6 rule both share).
"""
import math

import numpy as np

from geometry_ref import Box

CHUNK, BLOCK, WAVE = 4096, 256, 64
TOL = 2.0 ** -23


def _terms(xyz, box, idx, w_all):
    """the ten per-atom terms [10, n] of one set: w, w e (3), (w e_a) e_b for ab = xx xy xz yy yz zz"""
    x = [xyz[k].astype(np.float64) for k in range(3)]
    i0 = idx[0]
    ex, ey, ez = box.mi_f64(x[0][idx] - x[0][i0], x[1][idx] - x[1][i0], x[2][idx] - x[2][i0])
    w = w_all[idx].astype(np.float64)
    wx, wy, wz = w * ex, w * ey, w * ez
    return np.stack([w, wx, wy, wz, wx * ex, wx * ey, wx * ez, wy * ey, wy * ez, wz * ez])


def moments_pinned(xyz, box, idx, w_all):
    t = _terms(xyz, box, idx, w_all)
    n = t.shape[1]
    nch = (n + CHUNK - 1) // CHUNK
    pad = np.zeros((10, nch * CHUNK))
    pad[:, :n] = t
    pad = pad.reshape(10, nch, CHUNK // BLOCK, BLOCK)         # atom j of a chunk: step j // 256 of thread j % 256
    acc = np.zeros((10, nch, BLOCK))
    for k in range(CHUNK // BLOCK):
        acc = acc + pad[:, :, k, :]
    acc = acc.reshape(10, nch, BLOCK // WAVE, WAVE)
    lane = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ o]
    wave = acc[..., 0]
    blk = ((wave[..., 0] + wave[..., 1]) + wave[..., 2]) + wave[..., 3]
    s = blk[:, 0].copy()
    for ch in range(1, nch):
        s = s + blk[:, ch]
    return [float(v) for v in s]


def values_pinned(s):
    """Westin's measures from the ten sums, plain Python floats (IEEE fp64): M = S2 - (S1 S1^T) / W, cyclic Jacobi over the pairs
    (0,1), (0,2), (1,2), at most 16 sweeps, sorted, clamped at 0; t == 0 gives 0, 0, 0"""
    W = s[0]
    if W == 0.0:
        return 0.0, 0.0, 0.0
    a = [[0.0] * 3 for _ in range(3)]
    a[0][0] = s[4] - (s[1] * s[1]) / W; a[0][1] = s[5] - (s[1] * s[2]) / W; a[0][2] = s[6] - (s[1] * s[3]) / W
    a[1][1] = s[7] - (s[2] * s[2]) / W; a[1][2] = s[8] - (s[2] * s[3]) / W; a[2][2] = s[9] - (s[3] * s[3]) / W
    for _ in range(16):
        if (abs(a[0][1]) + abs(a[0][2])) + abs(a[1][2]) == 0.0:
            break
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = a[p][q]
            if apq == 0.0:
                continue
            theta = (a[q][q] - a[p][p]) / (2.0 * apq)
            t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
            if theta < 0.0:
                t = -t
            c = 1.0 / math.sqrt(t * t + 1.0)
            sn = t * c
            rp, rq = a[min(r, p)][max(r, p)], a[min(r, q)][max(r, q)]
            a[min(r, p)][max(r, p)] = c * rp - sn * rq
            a[min(r, q)][max(r, q)] = sn * rp + c * rq
            a[p][p] = a[p][p] - t * apq
            a[q][q] = a[q][q] + t * apq
            a[p][q] = 0.0
    l1, l2, l3 = a[0][0], a[1][1], a[2][2]
    if l1 < l2:
        l1, l2 = l2, l1
    if l2 < l3:
        l2, l3 = l3, l2
    if l1 < l2:
        l1, l2 = l2, l1
    l1, l2, l3 = (0.0 if v < 0.0 else v for v in (l1, l2, l3))
    t = (l1 + l2) + l3
    if t == 0.0:
        return 0.0, 0.0, 0.0
    return (l1 - l2) / t, (2.0 * (l2 - l3)) / t, (3.0 * l3) / t


def frame_plain(xyz, box, idx, w_all):
    t = _terms(xyz, box, idx, w_all)
    W = np.sum(t[0])
    if W == 0.0:
        return 0.0, 0.0, 0.0
    S1 = np.array([np.sum(t[1]), np.sum(t[2]), np.sum(t[3])])
    S2 = np.array([[np.sum(t[4]), np.sum(t[5]), np.sum(t[6])], [0.0, np.sum(t[7]), np.sum(t[8])], [0.0, 0.0, np.sum(t[9])]])
    S2 = S2 + np.triu(S2, 1).T
    M = S2 - np.outer(S1, S1) / W
    l3, l2, l1 = (max(float(v), 0.0) for v in np.linalg.eigvalsh(M))
    tt = l1 + l2 + l3
    if tt == 0.0:
        return 0.0, 0.0, 0.0
    return (l1 - l2) / tt, 2.0 * (l2 - l3) / tt, 3.0 * l3 / tt


def values(coords, box, sets, mass=None, geometric=False, flags=7, frames=None, pinned=True):
    """coords float32 [F, 3, N]; box as geometry_ref.Box takes it, or a list of one per frame; sets: one index array, or a list of P of
    them (one per context).  mass None or geometric=True: unit weights.  -> float32 [3, len(frames), P]: lin, plan, iso"""
    F, _, N = coords.shape
    sets = [np.asarray(sets, np.int64).reshape(-1)] if np.ndim(sets[0]) == 0 else [np.asarray(s, np.int64).reshape(-1) for s in sets]
    w = np.ones(N, np.float32) if (mass is None or geometric) else np.asarray(mass, np.float32)
    frames = range(F) if frames is None else list(frames)
    out = np.zeros((3, len(frames), len(sets)), np.float32)
    for k, f in enumerate(frames):
        bx = Box(box[f] if isinstance(box, list) else box, flags)
        for c, idx in enumerate(sets):
            v = values_pinned(moments_pinned(coords[f], bx, idx, w)) if pinned else frame_plain(coords[f], bx, idx, w)
            out[:, k, c] = np.asarray(v, np.float64).astype(np.float32)
    return out
