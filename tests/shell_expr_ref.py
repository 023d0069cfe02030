"""Yardstick of DESIGN 1.9 - and / or / not over within() shells.

It imports neither the package's evaluator nor the oracle.  Per frame and term, the outcomes h_i come from the numpy arithmetic of
tests/within_ref.py (wrap, pair_d - through its hits()), in the list order of T; under exclude_ref the atoms of R_i read h_i = 0 and stay
in T (DECISION D-EXPR-SELF).  An entry of T is a member iff bit sum(h_i << i) of the truth table is set.  For volumes, sdf() is
tests/shell_sdf_ref.py's loop over the frames with the membership supplied from here (the CPU oracle is handed in by the caller, as there).

A term is (R, r_min, r_max)."""
import numpy as np

import within_ref as W
import shell_sdf_ref as S
from geometry_ref import Box


def as_box(box, tilt=(0.0, 0.0, 0.0), flags=7):
    return box if isinstance(box, Box) else Box(S.box6(box, tilt), flags)


def outcomes(xyz, box, T, terms, closed=False, exclude_ref=False, slab=True):
    """one frame -> int [len(T)]: sum(h_i << i) of every list entry"""
    T = np.asarray(T, np.int64)
    idx = np.zeros(T.size, np.int64)
    for i, (ref, rmin, rmax) in enumerate(terms):
        h = W.hits(xyz, box, T, ref, rmin, rmax, closed, slab)
        if exclude_ref:
            h = h & ~np.isin(T, np.asarray(ref, np.int64))
        idx |= h.astype(np.int64) << i
    return idx


def lookup(idx, truth, k):
    """outcomes of k terms -> bool: the truth table's answer per entry"""
    assert 1 <= k <= 4 and 0 <= int(truth) < (1 << (1 << k))
    table = np.array([(int(truth) >> v) & 1 for v in range(1 << k)], bool)
    return table[idx]


def select(idx, which):
    """outcomes over a pool of terms -> the outcomes of the terms `which` (pool positions), renumbered 0, 1, ... in that order: several
    expressions over the same terms share one pass of within_ref.hits per term"""
    out = np.zeros_like(idx)
    for i, w in enumerate(which):
        out |= ((idx >> w) & 1) << i
    return out


def members(xyz, box, T, terms, truth, closed=False, exclude_ref=False, slab=True):
    """one frame -> bool [len(T)]: the members of the expression, in the list order of T"""
    return lookup(outcomes(xyz, box, T, terms, closed, exclude_ref, slab), truth, len(terms))


def counts(coords, box, T, terms, truth, tilt=(0.0, 0.0, 0.0), flags=7, frames=None, **kw):
    """coords float32 [F, 3, N] -> float32 [len(frames)]: the rows of the count form"""
    bx = as_box(box, tilt, flags)
    frames = range(coords.shape[0]) if frames is None else frames
    return np.array([members(coords[f], bx, T, terms, truth, **kw).sum() for f in frames], np.float32)


def atom_mask(xyz, box, T, terms, truth, n_atoms, **kw):
    """one frame -> bool [n_atoms]: the members by atom"""
    out = np.zeros(n_atoms, bool)
    out[np.asarray(T, np.int64)[members(xyz, box, T, terms, truth, **kw)]] = True
    return out


def sdf(O, coords, box, structures, mass, T, terms, truth, cutoff, tilt=(0.0, 0.0, 0.0), flags=7, frames=None, closed=False,
        exclude_ref=False, slab=True, dim=128):
    """shell_sdf_ref.shell_sdf with the members of the expression -> (volume u64[dim^3], populations int [len(frames)])"""
    frames = list(range(coords.shape[0])) if frames is None else list(frames)
    b6 = S.box6(box, tilt)
    bx = Box(b6, flags)
    ocell = O.make_cell(b6[:3], flags, b6[3:])
    structures = np.ascontiguousarray(structures, np.int32)
    smass = np.asarray(mass, np.float32)[structures]
    pose = O.sdf_ref_pose(coords[0, 0], coords[0, 1], coords[0, 2], ocell, structures[0], smass[0])
    vol = np.zeros(dim ** 3, np.uint64)
    pops = []
    T = np.asarray(T, np.int64)
    for f in frames:
        lst = T[members(coords[f], bx, T, terms, truth, closed, exclude_ref, slab)].astype(np.int32)
        pops.append(len(lst))
        if len(lst) == 0:
            continue
        _, R32, c32 = O.sdf_frame_align(coords[f, 0], coords[f, 1], coords[f, 2], ocell, structures, smass, pose)
        O.sdf_frame_scatter(coords[f, 0], coords[f, 1], coords[f, 2], ocell, structures, R32, c32, lst, cutoff, dim, vol)
    return vol, np.asarray(pops)


# truth tables of two terms (index = h_0 + 2 h_1) and the four-term case of the blob system
AND2, A_NOT_B, XOR2, OR2, NOT1 = 0b1000, 0b0010, 0b0110, 0b1110, 0b01


def table(fn, k):
    """the truth table of fn(h_0, ..., h_{k-1}) -> bool"""
    return sum(1 << v for v in range(1 << k) if fn(*[(v >> i) & 1 for i in range(k)]))
