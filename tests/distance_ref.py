"""Independent reference of the distance family (DESIGN S6) in numpy + the standard library.  It imports neither the package nor the
oracle.  Two layers:

Restatement (`com`): distance(a, b) step by step from the contract text - the S6 centres of both sets (geometry_ref.set_centres: fp64
sums in index order, de-periodised against the set's first atom, rounded to fp32), the fp32 minimum image of their difference by
rounding (Box.mi_f32), d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) and a correctly rounded fp32 square root.  Every step is IEEE-exact, so
the kernel must agree bit for bit.

Plain fp64 (`minmax`, `pair`): distance_min / _max / _pair in orthorhombic and open cells, written from scratch - the fp32 inputs are
converted exactly, d = x_i - x_j, d -= L * rint(d / L) on periodic axes, sqrt(sum d^2), min / max over all pairs.  No wrap step, no fp32
and no code shared with the restatement: Box.mi_f32 and fmaf are not used here.  The kernels wrap both atoms into the cell in fp32
first, so they agree only within `tolerance`.  For triclinic cells `min_images27` searches the 27 neighbouring images in fp64: the image
rule of the kernels (rint in fractional space) is discontinuous, so only a minimum well below the cell's width is comparable.
"""
import itertools

import numpy as np

import geometry_ref as G

EPS = 2.0 ** -24
UNITS = 16.0        # bound of the fp64 comparison in units of 2^-24 * M (orthorhombic and open cells)
UNITS_TRI = 32.0    # the same for the triclinic 27-image search (see tolerance_tri)


# ---- restatement ----------------------------------------------------------------------------------------------------------------------

def com_frame(xyz, box, a_sets, b_sets, mass):
    """one frame: xyz float32 [3, N], box a geometry_ref.Box, P index arrays per side, mass float32 [N] -> float32 [P]"""
    ca, cb = G.set_centres(xyz, box, a_sets, mass), G.set_centres(xyz, box, b_sets, mass)
    dx, dy, dz = box.mi_f32(ca[0] - cb[0], ca[1] - cb[1], ca[2] - cb[2])
    dx, dy, dz = (np.asarray(v, np.float32) for v in (dx, dy, dz))
    d2 = G.fmaf(dz, dz, G.fmaf(dy, dy, dx * dx))
    return np.sqrt(d2.astype(np.float32))           # numpy's float32 sqrt is correctly rounded


def com(coords, box, a_sets, b_sets, mass=None, flags=7, geometric=False, frames=None):
    """coords float32 [F, 3, N]; box as geometry_ref.Box takes it; a_sets / b_sets: lists of P index arrays.  mass None or
    geometric=True: unit weights (D-DIST-COM) -> float32 [len(frames), P]"""
    F, _, N = coords.shape
    a_sets = [np.asarray(s, np.int64).reshape(-1) for s in a_sets]
    b_sets = [np.asarray(s, np.int64).reshape(-1) for s in b_sets]
    m = np.ones(N, np.float32) if (mass is None or geometric) else np.asarray(mass, np.float32)
    bx = G.Box(box, flags)
    return np.stack([com_frame(coords[f], bx, a_sets, b_sets, m) for f in (range(F) if frames is None else frames)])


# ---- plain fp64 -----------------------------------------------------------------------------------------------------------------------

def _edges(box):
    """(Lx, Ly, Lz) as the fp32 values the library stores, in fp64; zeros for an open cell"""
    if box is None:
        return (0.0, 0.0, 0.0)
    if np.isscalar(box):
        box = (box,) * 3
    assert len(box) == 3 or not any(box[3:]), "triclinic cells have no plain fp64 reference: use min_images27"
    return tuple(float(np.float32(v)) for v in box[:3])


def pair_frame(xyz, box, flags, a, b):
    """all |a| x |b| distances of one frame in fp64, row-major (a outer): float64 [|a|, |b|]"""
    L = _edges(box)
    x = np.asarray(xyz, np.float32).astype(np.float64)
    a, b = np.asarray(a, np.int64).reshape(-1), np.asarray(b, np.int64).reshape(-1)
    s = np.zeros((a.size, b.size))
    for k in range(3):
        d = x[k][a][:, None] - x[k][b][None, :]
        if (flags >> k) & 1 and L[k] > 0.0:
            d = d - L[k] * np.rint(d / L[k])
        s += d * d
    return np.sqrt(s)


def pair(coords, box, flags, a, b):
    """float64 [F, |a| * |b|]"""
    return np.stack([pair_frame(coords[f], box, flags, a, b).reshape(-1) for f in range(coords.shape[0])])


def minmax(coords, box, flags, a, b, maxi):
    """float64 [F]"""
    return np.array([(np.max if maxi else np.min)(pair_frame(coords[f], box, flags, a, b)) for f in range(coords.shape[0])])


def magnitude(coords, box):
    """M of every frame: max(L_max, max |x|), float64 [F]"""
    return np.maximum(max(_edges(box)), np.abs(coords.astype(np.float64)).max(axis=(1, 2)))


def tolerance(coords, box):
    """|got - ref| <= 16 * 2^-24 * M per frame, M = max(L_max, max |x|).  The kernels wrap each atom into [0, L): one rounding at
    magnitude <= L and at most one +-L correction; two atoms, their difference and the image shift stay under 6 L 2^-24 per component,
    sqrt(3) times that over three components; the roundings of d2 and of the root add about 2.5 * 2^-24 * d.  Under 12 units in all; in
    an open cell only the difference, d2 and the root round.  float64 [F]"""
    return UNITS * EPS * magnitude(coords, box)


def units(got, ref, coords, box):
    """the deviation of got [F, ...] from ref in units of 2^-24 * M of the frame"""
    got = np.asarray(got, np.float32).astype(np.float64).reshape(coords.shape[0], -1)
    ref = np.asarray(ref, np.float64).reshape(coords.shape[0], -1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return np.abs(got - ref) / (EPS * magnitude(coords, box))[:, None]


# ---- triclinic: 27-image search -------------------------------------------------------------------------------------------------------

def cell_matrix(box6):
    """columns a = (x, 0, 0), b = (xy, y, 0), c = (xz, yz, z) from (x, y, z, xy, xz, yz), the fp32 values in fp64"""
    x, y, z, xy, xz, yz = (float(np.float32(v)) for v in box6)
    return np.array([[x, xy, xz], [0.0, y, yz], [0.0, 0.0, z]])


def cell_widths(box6):
    """distance between opposite faces, per lattice direction: volume / area of the face"""
    A = cell_matrix(box6)
    vol = abs(np.linalg.det(A))
    return np.array([vol / np.linalg.norm(np.cross(A[:, (k + 1) % 3], A[:, (k + 2) % 3])) for k in range(3)])


def min_images27(coords, box6, a, b):
    """minimum over all pairs and over the 27 images around the fractionally reduced difference, fp64: float64 [F].  Exact minimum
    image distance wherever it is below half the smallest cell width (the reduced difference is then at most one cell off)."""
    A = cell_matrix(box6)
    Ai = np.linalg.inv(A)
    shifts = np.array([A @ np.array(n, float) for n in itertools.product((-1, 0, 1), repeat=3)])        # [27, 3]
    a, b = np.asarray(a, np.int64).reshape(-1), np.asarray(b, np.int64).reshape(-1)
    out = []
    for f in range(coords.shape[0]):
        x = coords[f].astype(np.float64)
        d = (x[:, a][:, :, None] - x[:, b][:, None, :]).reshape(3, -1)                                  # [3, pairs]
        s = Ai @ d
        d = A @ (s - np.rint(s))
        best = np.full(d.shape[1], np.inf)
        for sh in shifts:
            e = d + sh[:, None]
            best = np.minimum(best, (e * e).sum(axis=0))
        out.append(np.sqrt(best.min()))
    return np.array(out)


def magnitude_tri(coords, box6):
    """M of a triclinic frame: max(|x|, the extent of the wrapped cell along x = Lx + |xy| + |xz|)"""
    x, y, z, xy, xz, yz = (abs(float(v)) for v in box6)
    return np.maximum(max(x + xy + xz, y + yz, z), np.abs(coords.astype(np.float64)).max(axis=(1, 2)))


def tolerance_tri(coords, box6):
    """|got - ref| <= 32 * 2^-24 * M, M = magnitude_tri.  The S3t wrap goes through fractional coordinates: s_z = z * fl(1 / Lz) carries
    about 3 roundings (the reciprocal, the product, the fold into [0, 1)), s_y and s_x inherit them through the tilts and add their own
    (about 4 and 4.5 units of 2^-24 for tilts of a quarter of the edge), and the way back adds three fused operations at the magnitude
    of the wrapped coordinate.  Per atom that is at most about 8, 5 and 3 units of 2^-24 * M in x, y and z, twice that for a pair
    (norm about 20), plus the difference, the shift, d2 and the root: about 24 in the worst case.  float64 [F]"""
    return UNITS_TRI * EPS * magnitude_tri(coords, box6)
