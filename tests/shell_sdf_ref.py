"""Yardstick of DESIGN 1.8 - sdf() whose target is a within() shell.

It imports neither the package's evaluator nor anything under test.  Per frame, the members of the shell come from the numpy arithmetic of
tests/within_ref.py (wrap, pair_d - through its hits()), in list order; the CPU oracle then aligns the reference structures of that frame
onto the pose of trajectory frame 0 (sdf_ref_pose / sdf_frame_align) and scatters only the members (sdf_frame_scatter).  A frame in which
the shell is empty adds no voxels.  The oracle's own switches (sdf_include_self) are whatever the caller has set with oracle.set_spec.

A target is (T, None) - the static list T - or (T, (R, r_min, r_max)) - the shell."""
import numpy as np

import within_ref as W
from geometry_ref import Box


def box6(box, tilt=(0.0, 0.0, 0.0)):
    b = (box,) * 3 if np.isscalar(box) else tuple(box)
    return tuple(float(v) for v in b) + tuple(float(v) for v in tilt)


def members(xyz, bx, target, closed=False, exclude_ref=False, slab=True):
    """one frame -> (the index list of the target in this frame, list order kept; bool [len(T')] over the list the shell is taken of)"""
    t, shell = target
    t = np.asarray(t, np.int64)
    if shell is None:
        return t.astype(np.int32), np.ones(t.size, bool)
    ref, rmin, rmax = shell
    if exclude_ref:
        t = t[~np.isin(t, np.asarray(ref, np.int64))]
    if t.size == 0:
        return t.astype(np.int32), np.zeros(0, bool)
    h = W.hits(xyz, bx, t, ref, rmin, rmax, closed, slab)
    return t[h].astype(np.int32), h


def atom_mask(xyz, bx, target, n_atoms, **kw):
    """one frame -> bool [n_atoms]: the members by atom"""
    out = np.zeros(n_atoms, bool)
    out[members(xyz, bx, target, **kw)[0]] = True
    return out


def shell_sdf(O, coords, box, structures, mass, target, cutoff, tilt=(0.0, 0.0, 0.0), flags=7, frames=None, closed=False,
              exclude_ref=False, slab=True, dim=128):
    """coords float32 [F, 3, N], structures [K, m] -> (volume u64[dim^3], populations int [len(frames)]).  The reference pose is that of
    trajectory frame 0 whatever `frames` says."""
    frames = list(range(coords.shape[0])) if frames is None else list(frames)
    b6 = box6(box, tilt)
    bx = Box(b6, flags)
    ocell = O.make_cell(b6[:3], flags, b6[3:])
    structures = np.ascontiguousarray(structures, np.int32)
    smass = np.asarray(mass, np.float32)[structures]
    pose = O.sdf_ref_pose(coords[0, 0], coords[0, 1], coords[0, 2], ocell, structures[0], smass[0])
    vol = np.zeros(dim ** 3, np.uint64)
    pops = []
    for f in frames:
        lst, _ = members(coords[f], bx, target, closed, exclude_ref, slab)
        pops.append(len(lst))
        if len(lst) == 0:
            continue
        _, R32, c32 = O.sdf_frame_align(coords[f, 0], coords[f, 1], coords[f, 2], ocell, structures, smass, pose)
        O.sdf_frame_scatter(coords[f, 0], coords[f, 1], coords[f, 2], ocell, structures, R32, c32, lst, cutoff, dim, vol)
    return vol, np.asarray(pops)
