"""Restatement of DESIGN 1.10 (backbone phi / psi and the Ramachandran density) in numpy, written out from the contract text.

Angles: tests/geometry_ref.py's dihedral of the four single-atom sets, in radians, with DECISION D-BB-ENDS applied (the angle that lacks
its neighbour is +0).  Binning: np.float32 arithmetic, one operation at a time (DECISION D-RAMA-BIN), with the skip rules.  It imports
neither the package nor the oracle.
"""
import numpy as np

import geometry_ref as G

DIM, CLASSES = 512, 4
f32 = np.float32


def links(nseg, range_offsets):
    """per segment: bit 0 = has a predecessor, bit 1 = has a successor - only inside its range"""
    off = np.asarray(range_offsets, np.int64)
    assert off[0] == 0 and off[-1] == nseg and (np.diff(off) > 0).all()
    link = np.full(nseg, 3, np.uint8)
    link[off[:-1]] &= 2
    link[off[1:] - 1] &= 1
    return link


def angles(coords, box, n, ca, c, range_offsets, flags=7):
    """coords float32 [F, 3, N]; box as geometry_ref.Box takes it -> float32 [F, nseg, 2] = {phi, psi} in radians"""
    n, ca, c = (np.asarray(v, np.int64) for v in (n, ca, c))
    nseg = n.size
    link = links(nseg, range_offsets)
    out = np.zeros((coords.shape[0], nseg, 2), np.float32)
    sp = np.flatnonzero(link & 1)
    if sp.size:     # phi(s) = dihedral(C[s-1], N[s], CA[s], C[s])
        sets = [[[i] for i in v] for v in (c[sp - 1], n[sp], ca[sp], c[sp])]
        out[:, sp, 0] = G.values(coords, box, sets, radians=True, flags=flags)
    sn = np.flatnonzero(link & 2)
    if sn.size:     # psi(s) = dihedral(N[s], CA[s], C[s], N[s+1])
        sets = [[[i] for i in v] for v in (n[sn], ca[sn], c[sn], n[sn + 1])]
        out[:, sn, 1] = G.values(coords, box, sets, radians=True, flags=flags)
    return out


def coord(a):
    """column (from phi) or row (from psi): fp32, every operation rounded on its own"""
    a = np.asarray(a, np.float32)
    scale = f32(1.0 / (2.0 * np.pi))
    u = (a * scale).astype(np.float32) + f32(0.5)
    return (u.astype(np.float32) * f32(DIM)).astype(np.float32).astype(np.uint32) & np.uint32(DIM - 1)


def bin(table, rama_class, link, rows=None, skip_ends=False):
    """table float32 [F, nseg, 2]; rows: which frames enter (None: all) -> (counts uint64 [512, 512, 4] as [y, x, class], sums uint64 [4])"""
    table = np.asarray(table, np.float32)
    F, nseg, _ = table.shape
    cls = np.asarray(rama_class, np.uint8)
    counts = np.zeros((DIM, DIM, CLASSES), np.uint64)
    sums = np.zeros(CLASSES, np.uint64)
    for f in (range(F) if rows is None else rows):
        phi, psi = table[f, :, 0], table[f, :, 1]
        go = (cls < CLASSES) & ~((phi == 0) & (psi == 0))
        if skip_ends:
            go &= np.asarray(link) == 3
        x, y = coord(phi), coord(psi)
        for s in np.flatnonzero(go):
            counts[y[s], x[s], cls[s]] += np.uint64(1)
            sums[cls[s]] += np.uint64(1)
    return counts, sums
