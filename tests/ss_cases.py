"""Inputs for the secondary-structure tests.

Random chains (rama_cases.chains) almost never form an H-bond.  By D-SS-CHAIN the kernels never look at covalent geometry, so `planted`
places atoms freely: every C=O points along -z (every amide H then sits 1 A above its N), and a bond (a, d) is planted with
O[a] = N[d] + (0, 0, 2.9), C[a] = O[a] + (0, 0, 1.23) - E = -2.90 kcal/mol.  The planted graph is made of motifs: runs of i -> i + 3 / 4 / 5
bonds, parallel and antiparallel ladders, single bridges, single turns; the segments of a motif's bond chain sit 3 A apart on a snake path,
so that partners pass the CA gate and other pairs of the motif stay above -0.5.  `ideal` builds backbones from (phi, psi) with standard
bond geometry (NeRF), `sheet` two such strands in two ranges.  Everything is wrapped into the cell atom by atom (rama_cases.wrap).
"""
import numpy as np

import rama_cases as RC

# bond lengths (A) and angles (degrees) of a standard peptide backbone
B_N_CA, B_CA_C, B_C_N, B_C_O = 1.458, 1.525, 1.329, 1.231
A_N_CA_C, A_CA_C_N, A_C_N_CA, A_CA_C_O = 111.0, 116.2, 121.7, 120.5


def _place(a, b, c, bond, angle, torsion):
    """NeRF: the point d with |cd| = bond, angle(b, c, d) = angle and dihedral(a, b, c, d) = torsion (degrees)"""
    t, p = np.radians(angle), np.radians(torsion)
    bc = (c - b) / np.linalg.norm(c - b)
    nv = np.cross(b - a, bc)
    nv /= np.linalg.norm(nv)
    m = np.cross(nv, bc)
    d2 = np.array([-bond * np.cos(t), bond * np.sin(t) * np.cos(p), bond * np.sin(t) * np.sin(p)])
    return c + d2[0] * bc + d2[1] * m + d2[2] * nv


def ideal(phi, psi, nres):
    """-> float64 [4 * nres, 3]: N, CA, C, O per residue, every residue with the same (phi, psi), omega = 180"""
    xyz = np.zeros((4 * nres, 3))
    n = np.array([0.0, 0.0, 0.0])
    ca = np.array([B_N_CA, 0.0, 0.0])
    c = _place(np.array([0.0, 1.0, 0.0]), n, ca, B_CA_C, A_N_CA_C, 0.0)
    for r in range(nres):
        if r:
            n = _place(xyz[4 * r - 4], xyz[4 * r - 3], xyz[4 * r - 2], B_C_N, A_CA_C_N, psi)
            ca = _place(xyz[4 * r - 3], xyz[4 * r - 2], n, B_N_CA, A_C_N_CA, 180.0)
            c = _place(xyz[4 * r - 2], n, ca, B_CA_C, A_N_CA_C, phi)
        xyz[4 * r], xyz[4 * r + 1], xyz[4 * r + 2] = n, ca, c
        xyz[4 * r + 3] = _place(n, ca, c, B_C_O, A_CA_C_O, psi + 180.0)
    return xyz


def backbone(nseg):
    r = np.arange(nseg, dtype=np.int32)
    return 4 * r, 4 * r + 1, 4 * r + 2, 4 * r + 3


def frames_of(xyz, box, tilt=(0.0, 0.0, 0.0), flags=7, shift=(-1.0, -1.5, -0.5)):
    """float64 [F, N, 3] or [N, 3] -> wrapped float32 [F, 3, N], moved so that the structure crosses the cell's origin faces"""
    xyz = np.asarray(xyz, np.float64)
    if xyz.ndim == 2:
        xyz = xyz[None]
    return RC.wrap(xyz + np.asarray(shift), box, tilt, flags).astype(np.float32).transpose(0, 2, 1).copy()


def _strand_frame(s):
    """axis (first to last CA), the mean C=O direction made perpendicular to it, and their cross product"""
    ca = s[1::4]
    ax = ca[-1] - ca[0]
    ax /= np.linalg.norm(ax)
    co = (s[3::4] - s[2::4])
    co = co * np.where(np.arange(len(co)) % 2 == 0, 1.0, -1.0)[:, None]      # the C=O of a strand alternate sides
    up = co.mean(axis=0)
    up -= ax * np.dot(up, ax)
    up /= np.linalg.norm(up)
    return ax, up, np.cross(ax, up)


def sheet(parallel, nres=8, gap=4.8):
    """two (-139, 135) strands `gap` A apart along the direction of their C=O bonds -> float64 [8 * nres, 3]: the second strand is the
    first moved (parallel), or turned round that direction through the strand's middle and moved (antiparallel: the strand runs the
    other way, its C=O keep their sides)"""
    s = ideal(-139.0, 135.0, nres)
    ax, up, nm = _strand_frame(s)
    if parallel:
        return np.concatenate([s, s + up * gap])
    mid = s[1::4].mean(axis=0)
    rel = s - mid
    t = mid - np.outer(rel @ ax, ax) + np.outer(rel @ up, up) - np.outer(rel @ nm, nm)
    return np.concatenate([s, t + up * gap])


# ---- planted bonds -------------------------------------------------------------------------------------------------------------------------

def _motifs(rng, nseg, forced):
    """-> list of bond lists [(a, d), ...]; forced motifs first"""
    out = list(forced)
    for _ in range(max(2, nseg // 4)):
        kind = rng.integers(0, 7)
        if kind <= 2:                                   # a run of i -> i + n bonds: helices, single turns
            n, m = 3 + kind, int(rng.choice([1, 1, 2, 3, 5]))
            s = int(rng.integers(0, max(1, nseg - n - m)))
            out.append([(i, i + n) for i in range(s, s + m) if i + n < nseg])
        elif kind <= 4:                                 # an antiparallel ladder (m = 1: a lone bridge)
            m = int(rng.choice([1, 2, 3, 4]))
            i0, j0 = sorted(rng.integers(1, max(2, nseg - 1), 2))
            out.append([b for t in range(m) if i0 + t + 2 < j0 - t for b in ((i0 + t, j0 - t), (j0 - t, i0 + t))])
        else:                                           # a parallel ladder
            m = int(rng.choice([1, 2, 3, 4]))
            i0, j0 = sorted(rng.integers(1, max(2, nseg - 1), 2))
            out.append([b for t in range(m) if i0 + t + 3 < j0 and j0 + t < nseg - 1 for b in ((i0 + t - 1, j0 + t), (j0 + t, i0 + t + 1))])
    return out


def forced_motifs(nseg, frame):
    """a ladder whose partner indices cross 63 | 64 and one that crosses 127 | 128 - parallel in even frames, antiparallel in odd ones -
    and a 5-turn whose bond crosses 63 | 64 (where nseg has room for them)"""
    out = []
    for edge, i0 in ((64, 8), (128, 30)):
        if nseg >= edge + 2:
            if frame % 2 == 0:      # par(i0 + t, edge - 3 + t)
                out.append([b for t in range(4) for b in ((i0 + t - 1, edge - 3 + t), (edge - 3 + t, i0 + t + 1))])
            else:                   # anti(i0 + t, edge - t)
                out.append([b for t in range(4) for b in ((i0 + t, edge - t), (edge - t, i0 + t))])
    if nseg >= 66:
        out.append([(60, 65)])
    return out


def layouts(nseg):
    """rama_cases.splits plus two halves: the one layout in which two ranges are long enough to bridge each other"""
    out = RC.splits(nseg)
    if nseg >= 6 and [0, nseg // 2, nseg] not in out:
        out.append([0, nseg // 2, nseg])
    return out


def planted_graph(rng, nseg, forced=()):
    """a set of bonds in which every segment accepts at most once and donates at most once -> dict donor-of-acceptor {a: d}"""
    don_of, acc_of = {}, {}
    for bonds in _motifs(rng, nseg, forced):
        ok = bonds and all(0 <= a < nseg and 0 < d < nseg and a != d and d != a + 1 and a not in don_of and d not in acc_of for a, d in bonds)
        ok = ok and len({a for a, _ in bonds}) == len(bonds) and len({d for _, d in bonds}) == len(bonds)
        if ok:
            for a, d in bonds:
                don_of[a], acc_of[d] = d, a
    return don_of


def _snake(k):
    """the k-th point of a boustrophedon path over a grid 3 points wide, spacing 3 A: consecutive points are 3 A apart"""
    row, col = divmod(k, 3)
    return np.array([3.0 * (col if row % 2 == 0 else 2 - col), 3.0 * row, 0.0])


def planted(seed, nseg, frames, box, tilt=(0.0, 0.0, 0.0), flags=7, forced=forced_motifs, spread=36.0):
    """-> coords float32 [frames, 3, 4 * nseg], (n, ca, c, o), graphs (one {a: d} per frame)"""
    rng = np.random.default_rng(seed)
    xyz = np.zeros((frames, 4 * nseg, 3))
    graphs = []
    up = np.array([0.0, 0.0, 1.0])
    for f in range(frames):
        g = planted_graph(rng, nseg, forced(nseg, f) if forced else ())
        graphs.append(g)
        acc_of = {d: a for a, d in g.items()}
        N = rng.uniform(0.0, spread, (nseg, 3))
        # the bond chains a -> d -> g[d] -> ... (paths first, then cycles) laid along snake paths
        seen = set()
        for s in [q for q in g if q not in acc_of] + list(g):
            if s in seen:
                continue
            chain, q = [], s
            while q is not None and q not in seen:
                chain.append(q)
                seen.add(q)
                q = g.get(q)
            origin = rng.uniform(0.0, spread, 3)
            for k, q in enumerate(chain):
                N[q] = origin + _snake(k) + rng.uniform(-0.2, 0.2, 3)
        O = N + np.array([3.1, 2.7, -4.2]) + rng.uniform(-0.3, 0.3, (nseg, 3))        # an oxygen nobody donates to: out of every H's reach
        for a, d in g.items():
            O[a] = N[d] + 2.9 * up
        xyz[f, 0::4] = N
        xyz[f, 1::4] = N + np.array([1.2, 0.8, 0.3])
        xyz[f, 2::4] = O + 1.23 * up
        xyz[f, 3::4] = O
    return frames_of(xyz, box, tilt, flags, shift=(-2.0, -2.0, -2.0)), backbone(nseg), graphs

