"""Yardstick of DESIGN 1.7 - rdf() whose arguments are within() shells.

It imports neither the package's evaluator nor anything under test.  Per frame, the members of a shell come from the numpy arithmetic of
tests/within_ref.py (wrap, pair_d - through its hits()); the histogram is the CPU oracle's rdf_frame on that frame with those lists, summed
over the frames; weights64 is the oracle's rdf_weights with the per-frame sizes (DECISION D-SHELL-NORM; shell_norm=True: the sizes of the
parent lists).  A frame in which a shell is empty adds neither counts nor weight.  The oracle's own switches (rdf_closed, rdf_norm,
rdf_raw) are whatever the caller has set with oracle.set_spec.

A side is (T, None) - the static list T - or (T, (R, r_min, r_max)) - the shell."""
import numpy as np

import within_ref as W
from geometry_ref import Box


def box6(box, tilt=(0.0, 0.0, 0.0)):
    b = (box,) * 3 if np.isscalar(box) else tuple(box)
    return tuple(float(v) for v in b) + tuple(float(v) for v in tilt)


def members(xyz, bx, side, closed=False, exclude_ref=False, slab=True):
    """one frame -> the index list of the side in this frame (list order kept)"""
    t, shell = side
    t = np.asarray(t, np.int64)
    if shell is None:
        return t.astype(np.int32)
    ref, rmin, rmax = shell
    if exclude_ref:
        t = t[~np.isin(t, np.asarray(ref, np.int64))]
    if t.size == 0:
        return t.astype(np.int32)
    return t[W.hits(xyz, bx, t, ref, rmin, rmax, closed, slab)].astype(np.int32)


def shell_rdf(O, coords, box, sides, rmin, rmax, tilt=(0.0, 0.0, 0.0), flags=7, frames=None, closed=False, exclude_ref=False,
              shell_norm=False, slab=True, method="brute"):
    """`method`: the oracle's rdf_frame by all pairs ("brute") or through its own cell list ("cells", for the full-size system).
    coords float32 [F, 3, N] -> (counts u64[1024], weights64 f64[1024], populations int [2][len(frames)])"""
    frames = list(range(coords.shape[0])) if frames is None else list(frames)
    b6 = box6(box, tilt)
    bx = Box(b6, flags)
    ocell = O.make_cell(b6[:3], flags, b6[3:])
    counts = np.zeros(1024, np.uint64)
    weights = np.zeros(1024, np.float64)
    pops = [[], []]
    for f in frames:
        lists = [members(coords[f], bx, s, closed, exclude_ref, slab) for s in sides]
        for k in range(2):
            pops[k].append(len(lists[k]))
        if min(len(v) for v in lists) == 0:
            continue
        O.rdf_frame(coords[f, 0], coords[f, 1], coords[f, 2], ocell, lists[0], lists[1], rmin, rmax, counts=counts, method=method)
        n = [len(sides[k][0]) if shell_norm else len(lists[k]) for k in range(2)]
        O.rdf_weights(ocell, n[0], n[1], rmin, rmax, weights=weights)
    return counts, weights, np.asarray(pops)
