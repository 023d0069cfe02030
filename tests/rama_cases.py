"""Seeded backbone chains for the Ramachandran tests: N, CA, C, O per residue, bond lengths 1.2 - 1.6 A, no three consecutive
atoms within 5 degrees of collinear (bond angles between 60 and 150 degrees), placed in a cell so that the chains cross its faces, every
atom wrapped into the cell on its own - the minimum image has to put the bonds back together."""
import numpy as np

ATOMS_PER_RESIDUE = 4


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _step(rng, prev):
    """a bond direction 30 .. 120 degrees off the previous one: the angle at the shared atom is 60 .. 150 degrees"""
    while True:
        d = _unit(rng)
        cs = float(np.dot(d, prev))
        if -0.5 <= cs <= 0.866:
            return d


def wrap(xyz, box, tilt=(0.0, 0.0, 0.0), flags=7):
    """xyz [..., 3] -> every atom into the cell on its own, along the periodic axes only (triclinic: in fractional space)"""
    L = np.asarray(box, np.float64)
    xy, xz, yz = tilt
    p = xyz.astype(np.float64).copy()
    sz = p[..., 2] / L[2]
    sy = (p[..., 1] - yz * sz) / L[1]
    sx = (p[..., 0] - xy * sy - xz * sz) / L[0]
    s = [sx, sy, sz]
    for k in range(3):
        if flags & (1 << k):
            s[k] = s[k] - np.floor(s[k])
    out = np.empty_like(p)
    out[..., 2] = s[2] * L[2]
    out[..., 1] = s[1] * L[1] + yz * s[2]
    out[..., 0] = s[0] * L[0] + xy * s[1] + xz * s[2]
    return out


def chains(seed, nseg, frames, box, tilt=(0.0, 0.0, 0.0), flags=7):
    """-> coords float32 [frames, 3, 4 * nseg] (atom 4 r + {0, 1, 2, 3} = N, CA, C, O of residue r), n, ca, c int32 [nseg].
    One covalent chain through all residues per frame (the ranges decide where phi / psi stop, not the geometry), started within 2 A
    of the cell's origin corner so that it crosses the faces; every frame is a chain of its own."""
    rng = np.random.default_rng(seed)
    xyz = np.zeros((frames, nseg * ATOMS_PER_RESIDUE, 3))
    for f in range(frames):
        pos = rng.uniform(-2.0, 2.0, 3)
        d = _unit(rng)
        for r in range(nseg):
            for k in range(3):                      # N, CA, C along the chain
                d = _step(rng, d)
                pos = pos + d * rng.uniform(1.2, 1.6)
                xyz[f, 4 * r + k] = pos
            xyz[f, 4 * r + 3] = pos + _step(rng, d) * rng.uniform(1.2, 1.6)      # the carbonyl O branches off C
    coords = wrap(xyz, box, tilt, flags).astype(np.float32).transpose(0, 2, 1).copy()
    r = np.arange(nseg, dtype=np.int32)
    return coords, 4 * r, 4 * r + 1, 4 * r + 2


def splits(nseg):
    """the range layouts of the size sweep: one range, {1, 2, 1, rest}, all ranges of length 1 (as offsets; duplicates dropped)"""
    out = [[0, nseg]]
    cut, off = [1, 2, 1], [0]
    for w in cut:
        if off[-1] + w >= nseg:
            break
        off.append(off[-1] + w)
    off.append(nseg)
    for o in (off, list(range(nseg + 1))):
        if o not in out:
            out.append(o)
    return out


def mixed_classes(nseg, seed=3):
    """general, glycine, proline, pre-proline and none, every class present once nseg >= 5"""
    cls = np.random.default_rng(seed).choice(np.array([0, 1, 2, 3, 255], np.uint8), nseg)
    cls[:min(nseg, 5)] = np.array([0, 1, 2, 3, 255], np.uint8)[:min(nseg, 5)]
    return cls
