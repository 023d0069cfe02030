"""Independent restatement of DESIGN 1.17 - connected clusters of groups per frame - in numpy.

It imports neither the package nor the oracle.  All pairs, no cells, fp32 operation by operation: the wrap of tests/within_ref.py and the
delta of tests/hbond_ref.py, the distance test of tests/contact_ref.py word for word.  One list of entries (atom, group):
  1. every entry is wrapped (SPEC S2 / S3t); an entry stands for the group the LIST gives it - there is no coincidence rule
     (D-CL-GEOMETRIC: coincident entries are at distance 0, so their groups are bonded anyway);
  2. entries i, j are in range when e = (i - j) - shift with the SPEC S3 / S3t image, d2 = fmaf(ez, ez, fmaf(ey, ey, ex ex)),
     d = sqrtf(d2), 0 <= d < r_cut (closed: <= r_cut);
  3. groups g != h are bonded in the frame iff some entry of g is in range of some entry of h; the clusters are the connected components
     of that graph over all G groups, made here with a plain sequential union-find (and cross-checked against SciPy's
     connected_components where SciPy can be imported).
Per frame: the number of clusters and the size of the largest as float32, the label of every group (the lowest group of its cluster).
The record: u64 [G + 1], row s - 1 the clusters of s groups summed over the evaluated frames, the last row the frames.
near: how many entry pairs (i < j, of different groups) lie within 4 ulp of r_cut."""
import numpy as np

from geometry_ref import Box
from hbond_ref import delta, ulps_between
from within_ref import fmaf, wrap

f32 = np.float32


def frame_bonds(xyz, box, atoms, groups, G, r_cut, closed=False, chunk=256):
    """one frame -> (the bonded group pairs as sorted unique keys lo * G + hi; near)"""
    atoms, groups = np.asarray(atoms, np.int64), np.asarray(groups, np.int64)
    r_cut = f32(r_cut)
    aw = wrap(xyz[:, atoms], box)
    keys = []
    near = 0
    for a in range(0, atoms.size, chunk):
        sl = slice(a, a + chunk)
        e = delta(box, aw[:, sl, None], aw[:, None, :])
        d2 = fmaf(e[2], e[2], fmaf(e[1], e[1], e[0] * e[0]))
        d = np.sqrt(d2.astype(np.float32))
        hit = (d <= r_cut) if closed else (d < r_cut)
        other = groups[sl, None] != groups[None, :]
        upper = np.arange(a, min(a + chunk, atoms.size))[:, None] < np.arange(atoms.size)[None, :]
        near += int((other & upper & (ulps_between(d, r_cut) <= 4)).sum())
        ii, jj = np.nonzero(hit & other & upper)
        gi, gj = groups[a + ii], groups[jj]
        keys.append(np.unique(np.minimum(gi, gj) * G + np.maximum(gi, gj)))
    return (np.unique(np.concatenate(keys)) if keys else np.zeros(0, np.int64)), near


def components(G, keys):
    """labels uint32 [G]: the lowest group of every group's component, by a plain union-find over the edges in the order given"""
    parent = list(range(G))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for k in keys.tolist():
        a, b = find(k // G), find(k % G)
        if a != b:
            parent[max(a, b)] = min(a, b)
    labels = np.array([find(g) for g in range(G)], np.uint32)
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return labels
    m = coo_matrix((np.ones(keys.size, np.int8), (keys // G, keys % G)), shape=(G, G))
    n, lab = connected_components(m, directed=False)
    lowest = np.full(n, G, np.int64)
    np.minimum.at(lowest, lab, np.arange(G))
    assert np.array_equal(lowest[lab].astype(np.uint32), labels), "the union-find and SciPy's components disagree"
    return labels


def evaluate(coords, box, atoms, groups, G, r_cut, closed=False, flags=7, frames=None):
    """coords float32 [F, 3, N]; frames: the evaluated frames in order, a frame named twice counts twice.
    -> dict(counts, largest float32 [F] (0 where not evaluated), record uint64 [G + 1], labels {frame: uint32 [G]}, near)"""
    F = coords.shape[0]
    frames = list(range(F)) if frames is None else list(frames)
    assert np.unique(np.asarray(groups)).size == G, "every group needs an entry"
    rec = np.zeros(G + 1, np.uint64)
    counts, largest = np.zeros(F, np.float32), np.zeros(F, np.float32)
    labels = {}
    near = 0
    for f in frames:
        bx = Box(box[f] if isinstance(box, list) else box, flags)
        keys, nd = frame_bonds(coords[f], bx, atoms, groups, G, r_cut, closed)
        near += nd
        lab = components(G, keys)
        sizes = np.bincount(lab, minlength=G)
        sizes = sizes[sizes > 0]
        counts[f], largest[f] = f32(sizes.size), f32(sizes.max())
        rec[:G] += np.bincount(sizes - 1, minlength=G).astype(np.uint64)
        rec[G] += np.uint64(1)
        labels[f] = lab
    return dict(counts=counts, largest=largest, record=rec, labels=labels, near=near)
