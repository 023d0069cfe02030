"""The systems of tests/test_hbond.py and tests/test_hbond_gpu.py: small, seeded, built once per process."""
import math

import numpy as np

f32 = np.float32
R_DA, ANGLE = 3.5, 150.0
# cubic, triclinic, a slab whose y axis is open: (box, tilt, periodic-axis flags)
CELLS = [((25.0, 25.0, 25.0), (0.0, 0.0, 0.0), 7), ((24.0, 22.0, 20.0), (5.0, -3.0, 4.0), 7), ((25.0, 18.0, 25.0), (0.0, 0.0, 0.0), 5)]
# one lane, the wave seam, the block seam
NPAIRS = [1, 63, 64, 65, 255, 256, 257]
# one entry, the LDS tile's quarter, and the three sizes around shell_brute_below (480), where the route changes
NACC = [1, 64, 65, 479, 480, 481]
# just large enough for a grid at R_DA (two pencils of 3.55 A per axis; 2.002 r < L), and too small for one (all pairs whatever is asked)
TIGHT, TOO_SMALL = 7.1, 6.9

_cache = {}


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


WATER = np.array([[0.0, 0.0, 0.0], [0.9572, 0.0, 0.0],
                  [0.9572 * math.cos(math.radians(104.52)), 0.9572 * math.sin(math.radians(104.52)), 0.0]])


def water_box(n_w, box, frames, seed=1, spread=1.3):
    """n_w waters, atoms O, H, H per molecule: oxygens uniform in the cell, spilling over its faces by `spread` - 1 (so that wrapping has
    work to do and hydrogens sit in other images than their donors), every molecule turned at random in every frame.
    -> coords float32 [F, 3, 3 n_w]"""
    key = ("water", n_w, tuple(np.atleast_1d(box)), frames, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        L = np.broadcast_to(np.asarray(box, float), (3,))
        out = []
        base = rng.uniform(-(spread - 1.0), spread, (n_w, 3)) * L
        for _ in range(frames):
            o = base + rng.normal(0.0, 0.4, (n_w, 3))
            mol = np.stack([WATER @ rotation(rng).T for _ in range(n_w)])
            out.append((o[:, None, :] + mol).reshape(-1, 3).T)
        _cache[key] = np.stack(out).astype(np.float32)
    return _cache[key]


def water_sites(n_w):
    """every O donates through both of its H and accepts: dict(donor, hydrogen, acceptor)"""
    o = np.arange(0, 3 * n_w, 3, dtype=np.int32)
    return dict(donor=np.repeat(o, 2), hydrogen=(np.repeat(o, 2) + np.tile([1, 2], n_w)).astype(np.int32), acceptor=o)


def subset_sites(n_w, npairs, nacc, seed):
    """npairs of the water box's pairs and nacc of its oxygens, in shuffled list order"""
    rng = np.random.default_rng(seed)
    s = water_sites(n_w)
    j = rng.permutation(2 * n_w)[:npairs]
    k = rng.permutation(n_w)[:nacc]
    return dict(donor=s["donor"][j], hydrogen=s["hydrogen"][j], acceptor=s["acceptor"][k])


def dimer(origin, rot=None):
    """Two waters with ONE hydrogen bond: O0-H1 ... O3 along the first water's x axis at 2.8 A (the angle at H1 is 180 degrees); the second
    water's hydrogens point away.  -> float64 [6, 3]"""
    a = WATER.copy()
    b = np.array([[2.8, 0.0, 0.0], [2.8 + 0.6, 0.75, 0.0], [2.8 + 0.6, -0.75, 0.0]])
    m = np.concatenate([a, b])
    if rot is not None:
        m = m @ rot.T
    return m + np.asarray(origin, float)


DIMER_SITES = dict(donor=np.array([0, 0, 3, 3], np.int32), hydrogen=np.array([1, 2, 4, 5], np.int32), acceptor=np.array([0, 3], np.int32))
DIMER_BOND = (0, 1, 3)
