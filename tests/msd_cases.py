"""Trajectories for the mean-squared displacement tests: coords float32 [F, 3, N] and the cells, one (box, tilt, flags) for
all frames or one per frame.  Frames hold WRAPPED coordinates: what the time unwrap has to undo."""
import numpy as np

CUBE8 = ((8.0, 8.0, 8.0), (0.0, 0.0, 0.0), 7)
OPEN_X = ((8.0, 8.0, 8.0), (0.0, 0.0, 0.0), 6)


def wrapped(pos, cells):
    """pos float64 [F, 3, N] unwrapped -> float32 [F, 3, N] folded into [0, L) along the periodic axes of every frame's cell"""
    F = pos.shape[0]
    cells = [cells] * F if isinstance(cells, tuple) else list(cells)
    out = np.array(pos, np.float64)
    for f in range(F):
        box, _, flags = cells[f]
        for k in range(3):
            if (flags >> k) & 1:
                out[f, k] = np.mod(out[f, k], box[k])
    return out.astype(np.float32)


def mover(F=40, step=(0.75, 0.0, 0.0), start=(0.5, 3.0, 5.0), cells=CUBE8, extra=0):
    """one atom that moves `step` per frame from `start` (and `extra` atoms at rest behind it), wrapped into the cell"""
    pos = np.zeros((F, 3, 1 + extra))
    pos[:, :, 0] = np.asarray(start)[None, :] + np.arange(F)[:, None] * np.asarray(step)[None, :]
    for j in range(extra):
        pos[:, :, 1 + j] = (1.0 + j, 2.0, 3.0)
    return wrapped(pos, cells)


def lattice_walk(n, F, seed, cells=CUBE8, natoms=None):
    """a seeded random walk on the lattice of 0.25 A: every coordinate, difference, product and sum of the query is exact in fp32, so a
    disagreement with the restatement is an indexing error, not rounding.  Steps of up to 1.5 A per axis and frame; natoms > n: the walkers
    are scattered among atoms at rest (the list is not the identity)."""
    rng = np.random.default_rng(seed)
    natoms = natoms or n
    pos = np.zeros((F, 3, natoms))
    pos[0] = rng.integers(0, 32, (3, natoms)) * 0.25
    steps = rng.integers(-6, 7, (F - 1, 3, natoms)) * 0.25
    atoms = np.sort(rng.permutation(natoms)[:n]).astype(np.int32)
    still = np.ones(natoms, bool)
    still[atoms] = False
    steps[:, :, still] = 0.0
    pos[1:] = pos[0] + np.cumsum(steps, axis=0)
    return wrapped(pos, cells), atoms


def breathing_cells(F, seed):
    """a cell that changes from frame to frame: edges on the 0.25 A lattice, between 7 and 9 A"""
    rng = np.random.default_rng(seed)
    return [(tuple(7.0 + 0.25 * rng.integers(0, 9, 3)), (0.0, 0.0, 0.0), 7) for _ in range(F)]


def liquid_walk(n, F, seed, box=(21.3, 19.7, 23.1)):
    """non-lattice fp32 coordinates: Gaussian steps of 0.6 A in an orthorhombic cell whose edges are not representable sums"""
    rng = np.random.default_rng(seed)
    pos = np.zeros((F, 3, n))
    pos[0] = rng.uniform(0.0, 1.0, (3, n)) * np.asarray(box)[:, None]
    pos[1:] = pos[0] + np.cumsum(rng.normal(0.0, 0.6, (F - 1, 3, n)), axis=0)
    cells = (box, (0.0, 0.0, 0.0), 7)
    return wrapped(pos, cells), cells
