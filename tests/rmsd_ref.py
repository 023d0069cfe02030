"""Two independent restatements of DESIGN 1.5 (rmsd) in numpy fp64.  Neither imports the package or the oracle.

pinned: the contract as the device evaluates it - integer link shifts along the index chain, their prefix sum, the offsets
        e_a = (x_a - x_0) + cart(k_a), the thirteen sums in the documented order (chunks of 4096 atoms, 256 threads that take every 256th
        atom, xor butterfly over the 64 lanes of a wave, the four waves, the chunks), Horn's 4x4 matrix, cyclic Jacobi in the documented
        pair order, the largest eigenvalue.  The emulator must agree with it bit for bit.
plain:  the same chain rule, np.sum moments, then another method altogether: weighted Kabsch by np.linalg.svd with the determinant
        correction and the residual summed directly, sum w |R p - q|^2 / W.  No eigenvalue formula.  bound() is the derived tolerance.
"""
import math

import numpy as np

from geometry_ref import Box

CHUNK, BLOCK, WAVE = 4096, 256, 64


def offsets(xyz, box, idx):
    """e_a [3, n] fp64 of one set in one frame: link shift n_a = -rint(frac(x_a - x_{a-1})), k_a = n_1 + ... + n_a (integers),
    e_a = (x_a - x_0) + cart(k_a)"""
    x = np.stack([xyz[k].astype(np.float64)[idx] for k in range(3)])
    n = x.shape[1]
    d = x[:, 1:] - x[:, :-1]
    L = [float(v) for v in box.L]
    shift = np.zeros((3, n), np.int64)
    if box.tri:
        xy, xz, yz = float(box.xy), float(box.xz), float(box.yz)
        sz = d[2] / L[2]
        sy = (d[1] - yz * sz) / L[1]
        sx = ((d[0] - xy * sy) - xz * sz) / L[0]
        for k, s in enumerate((sx, sy, sz)):
            shift[k, 1:] = -np.rint(s).astype(np.int64)
    else:
        for k in range(3):
            if box.p[k]:
                shift[k, 1:] = -np.rint(d[k] / L[k]).astype(np.int64)
    kk = np.cumsum(shift, axis=1).astype(np.float64)
    if box.tri:
        cart = [(kk[0] * L[0] + xy * kk[1]) + xz * kk[2], kk[1] * L[1] + yz * kk[2], kk[2] * L[2]]
    else:
        cart = [kk[k] * L[k] for k in range(3)]
    return np.stack([(x[k] - x[k][0]) + cart[k] for k in range(3)])


def pinned_sum(t):
    """[K, n] terms -> K sums in the device's order"""
    K, n = t.shape
    nch = (n + CHUNK - 1) // CHUNK
    pad = np.zeros((K, nch * CHUNK))
    pad[:, :n] = t
    pad = pad.reshape(K, nch, CHUNK // BLOCK, BLOCK)          # atom j of a chunk: step j // 256 of thread j % 256
    acc = np.zeros((K, nch, BLOCK))
    for k in range(CHUNK // BLOCK):
        acc = acc + pad[:, :, k, :]
    acc = acc.reshape(K, nch, BLOCK // WAVE, WAVE)
    lane = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ o]
    wave = acc[..., 0]
    blk = ((wave[..., 0] + wave[..., 1]) + wave[..., 2]) + wave[..., 3]
    s = blk[:, 0].copy()
    for ch in range(1, nch):
        s = s + blk[:, ch]
    return [float(v) for v in s]


def _moment_terms(e, w):
    wx, wy, wz = w * e[0], w * e[1], w * e[2]
    return [wx, wy, wz, (wx * e[0] + wy * e[1]) + wz * e[2]], (wx, wy, wz)


def jacobi4_max(A):
    """the largest diagonal entry after the device's cyclic Jacobi (vmd_jacobi4: pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), at most 24
    sweeps, columns then rows), plain Python floats"""
    A = [[float(v) for v in row] for row in A]
    for _ in range(24):
        off = 0.0
        for p in range(3):
            for q in range(p + 1, 4):
                off = off + abs(A[p][q])
        if off == 0.0:
            break
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(4):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = c * akp - s * akq
                    A[k][q] = s * akp + c * akq
                for k in range(4):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = c * apk - s * aqk
                    A[q][k] = s * apk + c * aqk
                A[p][q] = 0.0
                A[q][p] = 0.0
    return max(A[i][i] for i in range(4))


def finish_pinned(s, cst, n):
    """s: S1 (3), G, C (9, row-major C_ij = sum (w e_i) u_j); cst: W, U1 (3), Gu -> msd (fp64)"""
    W, U1, Gu = cst[0], cst[1:4], cst[4]
    if n <= 1 or W == 0.0:
        return 0.0
    Gp = s[3] - ((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]) / W
    Gq = Gu - ((U1[0] * U1[0] + U1[1] * U1[1]) + U1[2] * U1[2]) / W
    S = [[s[4 + 3 * i + j] - (s[i] * U1[j]) / W for j in range(3)] for i in range(3)]
    N = [[0.0] * 4 for _ in range(4)]
    N[0][0] = S[0][0] + S[1][1] + S[2][2]
    N[0][1] = S[1][2] - S[2][1]
    N[0][2] = S[2][0] - S[0][2]
    N[0][3] = S[0][1] - S[1][0]
    N[1][1] = S[0][0] - S[1][1] - S[2][2]
    N[1][2] = S[0][1] + S[1][0]
    N[1][3] = S[2][0] + S[0][2]
    N[2][2] = S[1][1] - S[0][0] - S[2][2]
    N[2][3] = S[1][2] + S[2][1]
    N[3][3] = S[2][2] - S[0][0] - S[1][1]
    for i in range(4):
        for j in range(i):
            N[i][j] = N[j][i]
    lam = jacobi4_max(N)
    msd = ((Gp + Gq) - 2.0 * lam) / W
    return 0.0 if msd < 0.0 else msd


def pose_pinned(xyz0, box0, idx, w_all):
    """(u [3, n], [W, U1x, U1y, U1z, Gu]) of one set at trajectory frame 0"""
    u = offsets(xyz0, box0, idx)
    w = w_all[idx].astype(np.float64)
    t, _ = _moment_terms(u, w)
    s = pinned_sum(np.stack(t + [w]))
    return u, [s[4], s[0], s[1], s[2], s[3]]


def frame_pinned(xyz, box, idx, w_all, u, cst):
    e = offsets(xyz, box, idx)
    w = w_all[idx].astype(np.float64)
    t, we = _moment_terms(e, w)
    for i in range(3):
        for j in range(3):
            t.append(we[i] * u[j])
    return math.sqrt(finish_pinned(pinned_sum(np.stack(t)), cst, len(idx)))


def frame_plain(xyz, box, idx, w_all, u):
    """(rmsd, (Gp + Gq) / W) by weighted Kabsch: centre both, SVD of the correlation matrix, determinant correction, direct residual"""
    n = len(idx)
    w = w_all[idx].astype(np.float64)
    W = np.sum(w)
    if n <= 1 or W == 0.0:
        return 0.0, 0.0
    e = offsets(xyz, box, idx)
    p = e - (e @ w / W)[:, None]
    q = u - (u @ w / W)[:, None]
    H = (p * w) @ q.T
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    R = Vt.T @ D @ U.T                                           # q ~ R p
    r = R @ p - q
    msd = np.sum(w * np.sum(r * r, axis=0)) / W
    scale = (np.sum(w * np.sum(p * p, axis=0)) + np.sum(w * np.sum(q * q, axis=0))) / W
    return math.sqrt(msd), float(scale)


def bound(ref, scale, n):
    """delta = max(n, 64) 2^-52 (Gp + Gq) / W is the rounding of the one-pass formula's msd; through the square root
    |sqrt a - sqrt b| <= min(|a - b| / sqrt b, sqrt |a - b|); 2^-23 ref covers the single rounding to fp32 on either side"""
    delta = max(n, 64) * 2.0 ** -52 * scale
    return 2.0 ** -23 * ref + (min(delta / ref, math.sqrt(delta)) if ref > 0.0 else math.sqrt(delta))


def values(coords, box, sets, mass=None, geometric=False, flags=7, frames=None, pinned=True, with_bound=False):
    """coords float32 [F, 3, N] (frame 0 = trajectory frame 0: the reference pose); box as geometry_ref.Box takes it, or a list of one
    per frame; sets: one index array, or a list of P of them.  mass None or geometric=True: unit weights.
    -> float32 [len(frames), P]; the row of frame 0 is +0 by definition.  with_bound (plain only): (values fp64, bounds)"""
    F, _, N = coords.shape
    sets = [np.asarray(sets, np.int64).reshape(-1)] if np.ndim(sets[0]) == 0 else [np.asarray(s, np.int64).reshape(-1) for s in sets]
    w = np.ones(N, np.float32) if (mass is None or geometric) else np.asarray(mass, np.float32)
    frames = range(F) if frames is None else list(frames)
    box_of = lambda f: Box(box[f] if isinstance(box, list) else box, flags)
    poses = [pose_pinned(coords[0], box_of(0), idx, w) for idx in sets]
    out = np.zeros((len(frames), len(sets)), np.float64)
    bnd = np.zeros((len(frames), len(sets)), np.float64)
    for k, f in enumerate(frames):
        if f == 0:
            continue
        bx = box_of(f)
        for c, idx in enumerate(sets):
            if pinned:
                out[k, c] = frame_pinned(coords[f], bx, idx, w, *poses[c])
            else:
                out[k, c], scale = frame_plain(coords[f], bx, idx, w, poses[c][0])
                bnd[k, c] = bound(out[k, c], scale, len(idx))
    if with_bound:
        return out, bnd
    return out.astype(np.float32)
