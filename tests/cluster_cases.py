"""The systems of tests/test_clusters.py and tests/test_clusters_gpu.py: small, seeded, built once per process."""
import numpy as np

import contact_cases as CC
import hbond_cases as HC

f32 = np.float32
R_CUT = 3.5
# contact_cases.chain is dense at 3.5 A (everything hangs together); at these radii its groups fall into clusters of many sizes
R_CHAIN, R_SWEEP = 2.4, 2.2
CELLS = HC.CELLS                 # cubic, triclinic, a slab whose y axis is open
TIGHT, TOO_SMALL = CC.TIGHT, CC.TOO_SMALL        # a cell with a grid at 3.5 A (two pencils per axis), and one without
SIZES = CC.SIZES                 # 1.16's (entries, groups); a pair with fewer entries than groups runs with as many groups as entries
LINES = [1, 2, 64, 65, 257, 481]
NEAR_STEP, FAR_STEP = 3.0, 6.0   # a line's spacing: neighbours inside r_cut and next-neighbours (2 x 3.0) outside it; everyone apart


def groups_for(n, G):
    """entry i of n -> group i Gc // n with Gc = min(G, n): contiguous groups, every one of them with an entry (a group without one is
    refused, so the pairs of contact_cases.SIZES with n < G keep their entries and run with n groups)"""
    Gc = min(G, n)
    return (np.arange(n, dtype=np.int64) * Gc // n).astype(np.int32), Gc


def sites(n, G, seed=0, shuffle=False):
    """the chain's atoms 0 .. n - 1 in contiguous groups; shuffle: the same entries in shuffled list order"""
    atoms = np.arange(n, dtype=np.int32)
    groups, Gc = groups_for(n, G)
    if shuffle:
        o = np.random.default_rng(seed).permutation(n)
        atoms, groups = atoms[o], groups[o]
    return dict(atoms=atoms, groups=groups, ngroups=Gc)


def one_per_group(n):
    return dict(atoms=np.arange(n, dtype=np.int32), groups=np.arange(n, dtype=np.int32), ngroups=n)


def line(G, step, frames=2, gap_at=None, x0=1.0):
    """G atoms on a straight line along x, `step` apart, at y = z = 5; gap_at = k: the spacing between atoms k - 1 and k is FAR_STEP.
    Every frame shifts the line by 0.25 A.  -> coords float32 [F, 3, G]"""
    x = x0 + step * np.arange(G, dtype=np.float64)
    if gap_at is not None:
        x[gap_at:] += FAR_STEP - step
    out = np.zeros((frames, 3, G))
    for f in range(frames):
        out[f, 0] = x + 0.25 * f
        out[f, 1:] = 5.0
    return out.astype(np.float32)


def line_cell(G, step, ring=False, gap=False):
    """a cell for line(): roomy beyond the line's ends, or - ring - exactly as long as the line with its closing bond (and its gap)"""
    length = step * G + (FAR_STEP - step if gap else 0.0)
    return ((length if ring else length + 40.0, 20.0, 20.0), (0.0, 0.0, 0.0), 7)


def ball(n, radius, frames, seed, centre=(12.0, 12.0, 12.0)):
    """n atoms uniform inside a ball -> coords float32 [F, 3, n]"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(frames, n, 3))
    v *= (radius * rng.uniform(0.0, 1.0, (frames, n, 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=2, keepdims=True)
    return (v + np.asarray(centre)).transpose(0, 2, 1).astype(np.float32)
