"""The systems of tests/test_contacts.py and tests/test_contacts_gpu.py: small, seeded, built once per process."""
import numpy as np

import hbond_cases as HC

f32 = np.float32
R_CUT, MIN_SEP = 4.5, 3
CELLS = HC.CELLS                 # cubic, triclinic, a slab whose y axis is open
# just large enough for a grid at TIGHT_R (two pencils of 3.55 A per axis; 2.002 r < L), and too small for one (all pairs whatever is asked)
TIGHT, TOO_SMALL, TIGHT_R = 7.1, 6.9, 3.5
# (entries, groups): one lane, the wave seam, the block seam, the three sizes around shell_brute_below (480), where the route changes;
# P = 1, 36 (the 32 / 33 word edge), 2016 (63 words exactly), 2080
SIZES = [(1, 2), (63, 9), (64, 64), (65, 65), (255, 2), (256, 9), (257, 64), (257, 65), (479, 9), (480, 65), (481, 64)]
NNATIVE = [1, 63, 64, 65]

_cache = {}


def chain(n, box, frames, seed=1, step=2.4, spread=1.15):
    """n atoms on a self-crossing random walk of `step` A (so that neighbours along the chain touch and distant ones meet again), started
    near a corner of the cell so that it spills over the faces, jittered frame by frame.  -> coords float32 [F, 3, n]"""
    key = ("chain", n, tuple(np.atleast_1d(box)), frames, seed, step)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        L = np.broadcast_to(np.asarray(box, float), (3,))
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        base = np.cumsum(d * step, axis=0)
        base = base - base.mean(axis=0) + (spread - 1.0) * L          # the walk's middle near the origin corner: every face is crossed
        out = [(base + rng.normal(0.0, 0.35, (n, 3))).T for _ in range(frames)]
        _cache[key] = np.stack(out).astype(np.float32)
    return _cache[key]


def contiguous_groups(n, G):
    """entry i of n -> group i G // n (n < G leaves groups without entries)"""
    return (np.arange(n, dtype=np.int64) * G // max(n, 1)).astype(np.int32)


def sites(n, G, seed=0, shuffle=False):
    """the chain's atoms 0 .. n - 1 with contiguous groups; shuffle: the same entries in shuffled list order"""
    atoms, groups = np.arange(n, dtype=np.int32), contiguous_groups(n, G)
    if shuffle:
        o = np.random.default_rng(seed).permutation(n)
        atoms, groups = atoms[o], groups[o]
    return dict(atoms=atoms, groups=groups, ngroups=G)


def min_sep_of(G):
    return min(MIN_SEP, G - 1)
