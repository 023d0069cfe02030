"""The systems of tests/test_rmsf.py and tests/test_rmsf_gpu.py: small, seeded, built once per process."""
import numpy as np

CHUNK = 4096
F = 5
N_ATOMS = 9100
# cubic, triclinic, a slab whose y axis is open: (box, tilt, periodic-axis flags)
CELLS = [((30.0, 30.0, 30.0), (0.0, 0.0, 0.0), 7), ((24.0, 22.0, 20.0), (5.0, -3.0, 4.0), 7), ((30.0, 12.0, 30.0), (0.0, 0.0, 0.0), 5)]
# 1: degenerate; 2, 3: a line, a plane; 63 / 64 / 65: the wave-per-set limit; 255 / 256 / 257: thread 0 owns a second atom; 4095 / 4096 /
# 4097: the chunk seam, its link and the carried-in shift; 8193: three chunks, the last of one atom
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
# unequal sets: all on the wave-per-set route; straddling it (small sets in a block launch); two chunk counts in one launch
POPULATIONS = [[3, 64, 40], [10, 65, 300], [64, CHUNK + 5, 700]]

_cache = {}


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def cloud(seed=1, n_atoms=N_ATOMS, frames=F):
    """An anisotropic cloud wider than every cell of CELLS, so that the index chain through it takes a shift at nearly every link; frame f
    is frame 0 turned about the cloud's centre, moved and jittered by 0.3 A - another set of shifts, the same molecule.
    -> (coords float32 [F, 3, n_atoms], mass float32 [n_atoms])"""
    key = ("cloud", seed, n_atoms, frames)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        base = rng.uniform(-6, 36, (n_atoms, 3)) * np.array([1.0, 0.5, 0.2])
        centre = base.mean(0)
        out = [base]
        for _ in range(1, frames):
            out.append((base - centre) @ rotation(rng).T + centre + rng.uniform(-4, 4, 3) + rng.normal(0.0, 0.3, (n_atoms, 3)))
        _cache[key] = (np.stack([p.T for p in out]).astype(np.float32), rng.uniform(1, 16, n_atoms).astype(np.float32))
    return _cache[key]


def subsets(seed, sizes, n_atoms=N_ATOMS):
    rng = np.random.default_rng(seed)
    return [rng.choice(n_atoms, n, replace=False).astype(np.int32) for n in sizes]


# where a link shift is planted: the first and the last lane of a wave, the last lane of a block's last wave, the first atom of the second
# chunk (the link across the seam), and its neighbour (the carry-in alone)
PLANTED_AT = [64, 127, 255, 256, CHUNK - 1, CHUNK, CHUNK + 1]


def planted(L=60.0, n=CHUNK + 300, frames=F, seed=7):
    """A compact random-walk chain that lies inside the cell: no link of it takes a shift, so every wave skips its scans.  In frames >= 1
    the chain is cut at the atoms of PLANTED_AT (frame f plants every position whose rank is not f modulo 3) and everything behind a cut
    is moved by one cell along an axis - the image the chain rule has to undo.  -> (coords with the cuts, coords without them)"""
    rng = np.random.default_rng(seed)
    walk = np.cumsum(rng.normal(0.0, 0.25, (n, 3)), axis=0)
    walk = walk - walk.mean(0)
    assert np.abs(walk).max() < 0.45 * L
    whole, cut = [], []
    for f in range(frames):
        p = walk + 0.5 * L + (rng.normal(0.0, 0.2, (n, 3)) + rng.uniform(-1.0, 1.0, 3) if f else 0.0)
        whole.append(p)
        c = p.copy()
        if f:
            for r, a in enumerate(PLANTED_AT):
                if r % 3 != f % 3:
                    c[a:, r % 3] += L * (1 if r % 2 else -1)
        cut.append(c)
    as32 = lambda frames_: np.stack([p.T for p in frames_]).astype(np.float32)
    return as32(cut), as32(whole)
