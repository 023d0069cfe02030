"""Independent reference of the SDF alignment stage (K3: k_sdf_ref_pose, k_sdf_align, k_sdf_group) in NumPy fp64 and the standard
library.  It imports neither the package nor the oracle, and shares no algorithm with the kernel: no unwrap routine, no sequential
sums, no Jacobi, no quaternion.

Made whole: every case generates its structures whole and keeps, per atom, the integer lattice vector n it added before storing the
fp32 coordinate.  The whole position of atom a is stored_a - A (n_a - n_root), A the cell matrix: the generated structure on the
periodic image whose root atom (atom 0, or the root of the bond tree) lies where it is stored.  `bond_fractions` is what a case asserts
to stay below 0.45, so that no rounding of a hop is anywhere near a tie.

Centre: sum(w x) / sum(w) by math.fsum over exact products (w has 24 bits: x is split into a 24 bit head and its remainder).
Rotation: weighted Kabsch - SVD of S[i][j] = sum w c_i r_j, R = V diag(1, 1, det) U^T, so that q = R (x - c) lies on the pose.
Conditioning: Horn's 4 x 4 matrix N of the same S, its eigenvalues by np.linalg.eigvalsh; the unit of every comparison is
u = 2^-52 |N|_F / (l1 - l2), the first-order change of the top eigenvector under a relative perturbation 2^-52 of N.

REF_UNITS is the distance of THIS reference from a 40-digit one (tests/test_sdf_align_emu.py: test_reference_against_40_digits, mpmath,
exact S from the same fp32 inputs, top eigenvector by mpmath.eigsy), over every well-conditioned (frame, structure) of the suite.  The
kernel's bound is UNITS = 4 REF_UNITS: the 24-sweep cyclic Jacobi applies up to 144 plane rotations where LAPACK factorises once."""
import itertools
import math

import numpy as np

EPS = 2.0 ** -52
REF_UNITS = 20.0         # measured worst: 15.28 u over the suite's 694 well-conditioned pairs (unwrap_chain cube 20, frame 0, structure 4);
                         # a prototype over 300 random structures of 3 to 200 atoms saw 19 u: the next round figure above both
UNITS = 4.0 * REF_UNITS
COND_MAX = 1.0e3         # |N|_F / (l1 - l2) of a case that compares the matrix itself


def cell_matrix(g9):
    """columns a = (x, 0, 0), b = (xy, y, 0), c = (xz, yz, z) of the nine-float box {L, 1 / L, xy, xz, yz}: the fp32 values in fp64"""
    x, y, z, _, _, _, xy, xz, yz = (float(np.float32(v)) for v in g9)
    return np.array([[x, xy, xz], [0.0, y, yz], [0.0, 0.0, z]])


def periodic_axes(pbc):
    return np.array([bool(pbc & 8) or bool((pbc >> a) & 1) for a in range(3)])


def whole(stored, n, A, root=0):
    """stored float32 [m, 3], n int [m, 3] -> float64 [m, 3]: the structure on the image of its root atom"""
    dn = (np.asarray(n, np.int64) - np.asarray(n, np.int64)[root]).astype(np.float64)
    return np.asarray(stored, np.float32).astype(np.float64) - dn @ A.T


def bond_fractions(w, parent, A, pbc):
    """largest |fractional component| over the hops atom -> parent (parent < 0: the root), periodic axes only"""
    worst = 0.0
    per = periodic_axes(pbc)
    Ai = np.linalg.inv(A)
    for a, p in enumerate(parent):
        if p >= 0:
            s = Ai @ (w[a] - w[p])
            worst = max(worst, float(np.abs(s[per]).max()) if per.any() else 0.0)
    return worst


def chain_parent(m):
    return np.arange(-1, m - 1)


def _split(x):
    hi = x.astype(np.float32).astype(np.float64)
    return hi, x - hi


def centre(w, x):
    """w float [m] (fp32 values), x float64 [m, 3] -> (centre float64 [3], sum |w x| / sum w per axis)"""
    w = np.asarray(w, np.float64)
    sw = math.fsum(w)
    c, mag = np.zeros(3), np.zeros(3)
    for k in range(3):
        hi, lo = _split(x[:, k])
        c[k] = math.fsum(np.concatenate([w * hi, w * lo])) / sw
        mag[k] = math.fsum(np.abs(w * x[:, k])) / sw
    return c, mag


def centre_bound(m, mag):
    """|c - c_ref| per axis of a sequential fp64 sum of m products and its division"""
    return (m + 2) * 2.0 ** -53 * mag


def horn(S):
    N = np.empty((4, 4))
    N[0, 0] = S[0, 0] + S[1, 1] + S[2, 2]
    N[1, 1] = S[0, 0] - S[1, 1] - S[2, 2]
    N[2, 2] = S[1, 1] - S[0, 0] - S[2, 2]
    N[3, 3] = S[2, 2] - S[0, 0] - S[1, 1]
    N[0, 1] = N[1, 0] = S[1, 2] - S[2, 1]
    N[0, 2] = N[2, 0] = S[2, 0] - S[0, 2]
    N[0, 3] = N[3, 0] = S[0, 1] - S[1, 0]
    N[1, 2] = N[2, 1] = S[0, 1] + S[1, 0]
    N[1, 3] = N[3, 1] = S[2, 0] + S[0, 2]
    N[2, 3] = N[3, 2] = S[1, 2] + S[2, 1]
    return N


class Fit:
    """one (frame, structure) against the pose"""
    pass


def fit(w, x, pose):
    """w [m], x float64 [m, 3] made whole, pose float64 [m, 3] centred -> Fit"""
    f = Fit()
    w = np.asarray(w, np.float64)
    f.m = x.shape[0]
    f.c, f.mag = centre(w, x)
    f.x = x
    d = x - f.c
    S = np.einsum("a,ai,aj->ij", w, d, pose)
    U, sv, Vt = np.linalg.svd(S)
    det = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0.0 else -1.0
    f.R = Vt.T @ np.diag([1.0, 1.0, det]) @ U.T
    f.S, f.N = S, horn(S)
    lam = np.linalg.eigvalsh(f.N)[::-1]
    f.normN = float(np.linalg.norm(f.N))
    gap = float(lam[0] - lam[1])
    f.cond = f.normN / gap if gap > 0.0 else math.inf
    f.u = EPS * f.cond
    f.e_opt = math.fsum(w * (d * d).sum(1)) + math.fsum(w * (pose * pose).sum(1)) - 2.0 * (sv[0] + sv[1] + det * sv[2])
    f.M = np.concatenate([f.R, -(f.R @ f.c)[:, None]], axis=1)
    return f


def residual(w, R, c, x, pose):
    """E(R) = sum w |R (x - c) - r|^2 in fp64"""
    q = (x - c) @ np.asarray(R, np.float64).T - pose
    return math.fsum(np.asarray(w, np.float64) * (q * q).sum(1))


def pose_of(w, x):
    """the centred pose of structure 0 of frame 0 -> (pose float64 [m, 3], centre, mag)"""
    c, mag = centre(w, x)
    return x - c, c, mag


def min_image27(d, A, per):
    """length of the shortest image of the displacement d, fp64: the fractionally reduced d and its 26 neighbours (periodic axes)"""
    Ai = np.linalg.inv(A)
    s = Ai @ d
    s = np.where(per, s - np.rint(s), s)
    best = math.inf
    for n in itertools.product((-1, 0, 1), repeat=3):
        n = np.where(per, np.array(n, float), 0.0)
        e = A @ (s + n)
        best = min(best, float(np.sqrt(e @ e)))
    return best
