"""A restatement of DESIGN 1.13 (rmsf) in numpy fp64.  It imports neither the package nor the oracle.

The chain rule that makes a set whole is DESIGN 1.5's, taken from tests/rmsd_ref.py (offsets).  The fit is another method than the
device's: weighted Kabsch by np.linalg.svd with the determinant correction, no quaternion, no Jacobi.  The residual
d_a = R (e_a - ebar) - (u_a - ubar) is quantised per frame with np.rint (nearest even, as the device's conversion) and the sums are
held in Python integers, so nothing here can overflow or round.  bound() is the derived tolerance of a comparison with the device."""
import math

import numpy as np

from geometry_ref import Box
import rmsd_ref as RM

ONE = 2.0 ** 24            # one Angstrom (one square Angstrom) in quanta, D-RMSF-FIXED
D2_MAX = 2.0 ** 20         # where q2 saturates
EPS = 2.0 ** -52


def horn(S):
    """Horn's symmetric 4 x 4 matrix of a 3 x 3 correlation matrix (only its eigenvalues are used here: the gap of bound())"""
    return np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                     [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                     [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], S[1, 1] - S[0, 0] - S[2, 2], S[1, 2] + S[2, 1]],
                     [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], S[2, 2] - S[0, 0] - S[1, 1]]])


def residual(e, u, w):
    """d [3, n] of one set in one frame and what bound() needs of the fit.  None: a degenerate set (D-RMSF-DEGENERATE), d = 0"""
    n = e.shape[1]
    W = float(np.sum(w))
    if n <= 1 or W == 0.0:
        return None
    ebar, ubar = e @ w / W, u @ w / W
    p, q = e - ebar[:, None], u - ubar[:, None]
    H = (p * w) @ q.T                                            # S of DESIGN 1.5's finish: S_ij = sum w p_i q_j
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    R = Vt.T @ D @ U.T                                           # q ~ R p, a proper rotation
    d = R @ p - q
    # for the bound: the size of the terms the device's nine C sums are made of, and the eigenvalues of N
    ne, nu = np.sqrt(np.sum(e * e, axis=0)), np.sqrt(np.sum(u * u, axis=0))
    terms = float(np.sum(w * ne * nu)) + float(np.linalg.norm(e @ w) * np.linalg.norm(u @ w)) / W
    lam = np.sort(np.linalg.eigvalsh(horn(H)))[::-1]
    return d, dict(p=np.sqrt(np.sum(p * p, axis=0)), q=np.sqrt(np.sum(q * q, axis=0)), terms=terms, lam=lam, n=n,
                   extent=float(ne.max() + nu.max()))


def bound(d, fit):
    """What one frame may add to the difference between a device accumulator and this restatement's, in quanta: [n] for the columns
    0..2 and [n] for column 3.

    (a) One quantum, for a rounding that falls the other way: |rint(x + t) - rint(x)| <= |t| + 1.
    (b) t, the difference of the two residuals.  Both sides compute d = R p - q in fp64; what differs is R.  The device's R is the
        rotation of the eigenvector of Horn's N for its largest eigenvalue.  N is linear in the nine sums C_ij - S1_i U1_j / W, each an
        n-term fp64 sum (rounding: K = max(n, 64) units of 2^-52 of the sum of the terms' sizes, `terms`; the floor of 64 stands for
        the few dozen roundings of the Jacobi sweeps), an entry of N is made of at most three of them, and N has 16
        entries: ||dN||_F <= 4 x 3 K 2^-52 terms.  By the Davis-Kahan theorem the eigenvector turns by at most ||dN|| / gap, gap =
        lambda_1 - lambda_2, and the rotation by twice the quaternion's angle: theta <= 24 K 2^-52 terms / gap.  The restatement's own
        SVD is granted the same, hence 48.  Where lambda_2 equals lambda_1 to within 64 x 2^-52 ||N|| the set is collinear in both
        frames (S has rank one), every eigenvector of that plane gives the same R p, and the gap is the one to the next eigenvalue.
        No eigenvalue apart from lambda_1 at all: N = 0, R is arbitrary, theta = pi.
        |t_a| <= theta |p_a| + the centroids' rounding (K 2^-52 of the set's extent, twice) + the dozen roundings of d itself.
    Column 3: |d + t|^2 - |d|^2 <= 2 |d| |t| + |t|^2."""
    K = max(fit["n"], 64)
    lam = fit["lam"]
    tol = 64 * EPS * max(abs(lam[0]), abs(lam[-1]))
    below = [v for v in lam[1:] if lam[0] - v > tol]
    theta = min(math.pi, 48 * K * EPS * fit["terms"] / (lam[0] - below[0])) if below else math.pi
    t = theta * fit["p"] + 2 * K * EPS * fit["extent"] + 12 * EPS * (fit["p"] + fit["q"])
    dn = np.sqrt(np.sum(d * d, axis=0))
    return 1.0 + ONE * t, 1.0 + ONE * (2.0 * dn * t + t * t)


def quantise(d):
    """-> (int64 [3, n], int64 [n]): q(d) per axis and q2(|d|^2) of one frame"""
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return np.rint(d * ONE).astype(np.int64), np.rint(np.minimum(d2, D2_MAX) * ONE).astype(np.int64)


def record(coords, box, sets, mass=None, geometric=False, flags=7, frames=None):
    """coords float32 [F, 3, N] (frame 0 = trajectory frame 0: the pose); box as geometry_ref.Box takes it, or a list of one per frame;
    sets: one index array or a list of P of them; frames: the trajectory frames accumulated (each as often as it is listed).
    -> (acc: object array [ntot + 1, 4] of Python integers - the signed sums of q(d) per axis, the sum of q2, the frame count in the
    last row -, bnd: float64 [ntot, 4], the allowed difference of every accumulator in quanta)"""
    F, _, N = coords.shape
    sets = [np.asarray(sets, np.int64).reshape(-1)] if np.ndim(sets[0]) == 0 else [np.asarray(s, np.int64).reshape(-1) for s in sets]
    w_all = np.ones(N, np.float32) if (mass is None or geometric) else np.asarray(mass, np.float32)
    frames = list(range(F)) if frames is None else list(frames)
    box_of = lambda f: Box(box[f] if isinstance(box, list) else box, flags)
    ntot = sum(len(s) for s in sets)
    acc = np.zeros((ntot + 1, 4), object)
    acc[...] = 0
    bnd = np.zeros((ntot, 4), np.float64)
    k0 = 0
    for idx in sets:
        n = len(idx)
        w = w_all[idx].astype(np.float64)
        u = RM.offsets(coords[0], box_of(0), idx)
        for f in frames:
            if f == 0:
                continue                                         # d = 0 by construction: the frame counts and adds nothing
            fit = residual(RM.offsets(coords[f], box_of(f), idx), u, w)
            if fit is None:
                continue
            q, q2 = quantise(fit[0])
            b, b2 = bound(*fit)
            for a in range(n):
                for k in range(3):
                    acc[k0 + a, k] += int(q[k, a])
                acc[k0 + a, 3] += int(q2[a])
            bnd[k0:k0 + n, :3] += b[:, None]
            bnd[k0:k0 + n, 3] += b2
        k0 += n
    acc[ntot, 0] = len(frames)
    return acc, bnd


def signed(got):
    """a device record uint64 [ntot + 1, 4] as Python integers: the columns 0..2 read as two's complement"""
    got = np.asarray(got, np.uint64)
    out = np.zeros(got.shape, object)
    out[:, :3] = got[:, :3].view(np.int64).astype(object)
    out[:, 3] = got[:, 3].astype(object)
    out[-1, :] = got[-1, :].astype(object)
    return out


def read(got):
    """vmd_eval_rmsf's formula applied to a record in numpy, operation for operation -> (rmsf [ntot], mean_dev [ntot, 3], frames)"""
    got = np.asarray(got, np.uint64)
    F = int(got[-1, 0])
    ntot = got.shape[0] - 1
    if F == 0:
        return np.zeros(ntot), np.zeros((ntot, 3)), 0
    scale = ONE * float(F)
    m = got[:-1, :3].view(np.int64).astype(np.float64) / scale
    msf = got[:-1, 3].astype(np.float64) / scale - ((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
    return np.sqrt(np.maximum(msf, 0.0)), m, F
