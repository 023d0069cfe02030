"""Pair distances ON the bin edges of rdf(): systems built from tests/rdf_ref.py, for the SIMT emulator (test_bin_edges_emu.py) and the
product library on the device (test_bin_edges_gpu.py).  The u64 counts of every route are held against the fp32 tier of rdf_ref with
assert_array_equal - after frame 0 and after frame 1 - and nothing on the device side has a tolerance.

A system belongs to one (cell, range) and has two frames over the same atoms; reference and target are every atom.

Frame 0, intended distances.  For every edge e_b = fl(r_min + b (r_max - r_min) / 1024), b = 0..1024, one pair at e_b, one at the float
below and one at the float above; at r_min and r_max also at +-2 and +-3 floats (distances that are not positive and normal are left
out: with r_min = 0 the pair on the edge is an atom with itself, d = 0).
  orthorhombic cells: the two atoms of a pair lie on a line along x, y or z and share the other two coordinates bit for bit.  Going up
      the line the anchor's coordinate is 0 and the satellite's is d; going down the anchor sits at P = 2^(e+1) for d in [2^e, 2^(e+1))
      and the satellite at P - d, a multiple of ulp(d) below 2^(e+1).  Every coordinate is an fp32 number inside the cell, the wrap
      (S2) leaves it alone, the subtraction is exact, d2 = fl(d d) and sqrtf gives d back.
  the triclinic cell: its wrap goes through fractional coordinates and rounds, so nothing can be laid down exactly.  Six satellites
      around an anchor, random directions, kept by rejection: a satellite stays iff the reference's d IS the intended float.
Frame 1, general d2.  Pairs in random directions whose reference d lies within +-4 floats of an edge (rejection), one pair per edge at
least; the atoms left over are spent on pairs ACROSS a periodic face (in the triclinic cell the sheared z face), kept only if the
reference takes a lattice image for them.  Their d2 is a sum of three rounded squares, not a rounded square.

coverage() asserts all of that from the reference alone, before anything is evaluated, and prints per system how many ordered pairs
the device's fast path has to park (t* within delta of an integer, delta of vmd_make_binning restated in rdf_ref.fast_delta) and how
many lie within the exact tier's margin of an integer.

Cells: the 39 A cube of pencil_loop_cases (3 x 3 pencils), its triclinic cell, and a cube of 2.001 r_max, too small for a grid
(2 r_max 1.001 is the least), which k_rdf_brute serves.  Routes are asserted from the launch profile (cases._kernel_family)."""
import numpy as np

import cases
import rdf_ref as R
import viamd_amd as V
from geometry_ref import Box
from test_within import options

f32 = np.float32

RANGES = {                                                  # name -> (r_min, r_max, the fast path is usable)
    "0:12": (0.0, 12.0, True),                              # the folded pop, r_min == 0
    "0:3.2": (0.0, 3.2, True),                              # most fp32 / exact disagreements
    "2.5:9": (2.5, 9.0, True),                              # vmd_pop_hot, fast_c != 0
    "11.9:12": (11.9, 12.0, True),                          # delta = 0.074
    "11.97:12": (11.97, 12.0, True),                        # delta just below 0.25
    "11.971:12": (11.971, 12.0, False),                     # delta just above 0.25: the degenerate branch
    "12-6ulp:12": (12.0 - 6 * 2.0 ** -20, 12.0, False),     # six floats wide: every hit sits in one of five bins
}
TRICLINIC = (52.0, 50.0, 49.0, 6.0, -4.0, 5.0)              # pencil_loop_cases._triclinic
CELLS = ("cube_39", "triclinic", "small")
TOL1 = 4                                                    # frame 1: floats around an edge


def cell_box(cell, rmax):
    return 39.0 if cell == "cube_39" else TRICLINIC if cell == "triclinic" else float(f32(2.001 * float(f32(rmax))))


def edges(rmin, rmax):
    lo, hi = float(f32(rmin)), float(f32(rmax))
    return (lo + np.arange(R.NBINS + 1) * (hi - lo) / R.NBINS).astype(np.float32)


def step(x, k):
    """the k-th float above (k > 0) or below x"""
    x = np.asarray(x, np.float32).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf if k > 0 else -np.inf))
    return x


def floats_apart(a, b):
    """a - b in floats (both positive)"""
    return np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64)


def intended(rmin, rmax):
    """the distances of frame 0, float32, ascending"""
    e = edges(rmin, rmax)
    v = [step(e, k) for k in (-1, 0, 1)] + [step(e[[0, -1]], k) for k in (-3, -2, 2, 3)]
    v = np.unique(np.concatenate(v))
    return v[v >= f32(2.0 ** -40)]


def _cell_matrix(box):
    b = (box,) * 3 if np.isscalar(box) else tuple(box)
    b = b + (0.0,) * (6 - len(b))
    return np.array([[b[0], b[3], b[4]], [0.0, b[1], b[5]], [0.0, 0.0, b[2]]])


def _lines(targets, span):
    """frame 0 of an orthorhombic cell -> (pos float64 [N, 3], i, j): pair k is (i[k], j[k]) at targets[k]"""
    trans = ((np.arange(4) + 0.5) * span / 4.0).astype(np.float32).astype(np.float64)
    pos, anchors, I, J = [], {}, [], []
    for k, d in enumerate(targets.astype(np.float64)):
        axis, down, line = k % 3, (k // 3) % 2, (k // 6) % 16
        P = 2.0 ** (np.floor(np.log2(d)) + 1.0) if down else 0.0
        p = np.zeros(3)
        p[(axis + 1) % 3], p[(axis + 2) % 3] = trans[line % 4], trans[line // 4]
        p[axis] = P
        key = (axis, line, P)
        if key not in anchors:
            anchors[key] = len(pos)
            pos.append(p.copy())
        p[axis] = P - d if down else d
        I.append(anchors[key]); J.append(len(pos))
        pos.append(p)
    pos = np.array(pos)
    assert np.array_equal(pos.astype(np.float32).astype(np.float64), pos), "a coordinate of frame 0 is no fp32 number"
    return pos, np.array(I), np.array(J)


def _directions(rng, shape):
    v = rng.normal(size=shape + (3,))
    return v / np.linalg.norm(v, axis=-1)[..., None]


def _reject(rng, bx, A, t, tol, anchors=None, face=False, rounds=40, M=48):
    """for every intended distance t[k] an (anchor, satellite) whose reference distance is within `tol` floats of it.
    anchors float64 [n, 3]: given, only the direction is drawn.  face: the anchor lies within 0.3 t of a periodic face (the z face of a
    triclinic cell) and the satellite beyond it.  -> (anchor [n, 3], satellite [n, 3] float32, found bool [n])"""
    n = t.size
    t64 = t.astype(np.float64)
    out_a, out_s, found = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, bool)
    Ld = np.diag(A)
    for _ in range(rounds):
        idx = np.nonzero(~found)[0]
        if idx.size == 0:
            break
        tt = t64[idx][:, None, None]
        if anchors is not None:
            a = np.broadcast_to(anchors[idx][:, None, :], (idx.size, M, 3)).copy()
        else:       # near the origin, where the coordinates' floats are as fine as the distance's; from 1 A on anywhere in the cell
            a = np.where(tt >= 1.0, rng.uniform(size=(idx.size, M, 3)) @ A.T, tt * (1.0 + 0.9 * rng.uniform(size=(idx.size, M, 3))))
        dirs = _directions(rng, (idx.size, M))
        if face:
            ax = np.full((idx.size, M), 2) if bx.tri else rng.integers(0, 3, (idx.size, M))
            if bx.tri:
                s = rng.uniform(0.1, 0.9, (idx.size, M, 3))
                s[..., 2] = 1.0 - rng.uniform(0.0, 0.3, (idx.size, M)) * tt[..., 0] / Ld[2]
                a = s @ A.T
            else:
                a = rng.uniform(0.1, 0.9, (idx.size, M, 3)) * Ld
                on = Ld[ax] - rng.uniform(0.0, 0.3, (idx.size, M)) * tt[..., 0]
                np.put_along_axis(a, ax[..., None], on[..., None], 2)
            up = np.abs(np.take_along_axis(dirs, ax[..., None], 2))
            np.put_along_axis(dirs, ax[..., None], up, 2)
        s_ = a + tt * dirs
        a32, s32 = a.reshape(-1, 3).astype(np.float32), s_.reshape(-1, 3).astype(np.float32)
        d = R.d_of(bx, a32.T, s32.T).reshape(idx.size, M)
        ok = np.abs(floats_apart(d, np.broadcast_to(t[idx][:, None], d.shape))) <= tol
        if face:
            ok &= _crosses(bx, A, a32, s32).reshape(idx.size, M)
        first = ok.argmax(axis=1)
        got = ok.any(axis=1)
        sel = idx[got]
        out_a[sel] = a32.reshape(idx.size, M, 3)[got, first[got]]
        out_s[sel] = s32.reshape(idx.size, M, 3)[got, first[got]]
        found[sel] = True
    return out_a, out_s, found


def _crosses(bx, A, a32, s32):
    """does the reference take a lattice image for the pair?  From the wrapped positions it sees: their difference is more than half a
    cell in fractional coordinates"""
    import within_ref as W
    wa, ws = W.wrap(a32.T, bx).astype(np.float64), W.wrap(s32.T, bx).astype(np.float64)
    frac = np.linalg.solve(A, wa - ws)
    return (np.abs(np.rint(frac)) >= 1.0).any(axis=0)


class System:
    def __init__(self, cell, rname):
        self.cell, self.rname = cell, rname
        self.rmin, self.rmax, self.fast = RANGES[rname]
        self.box = cell_box(cell, self.rmax)
        self.bx = Box(self.box, 7)
        A = _cell_matrix(self.box)
        rng = np.random.default_rng(1000 * CELLS.index(cell) + list(RANGES).index(rname) + 7)
        t0 = intended(self.rmin, self.rmax)
        while t0.size < 1200:                                    # a range of a few floats: every distance many times
            t0 = np.concatenate([t0, t0])
        # ---- frame 0
        if self.bx.tri:
            n_star = (t0.size + 5) // 6
            lead = t0[::6].astype(np.float64)[:n_star, None]
            anc = np.where(lead >= 1.0, rng.uniform(size=(n_star, 3)) @ A.T, lead * (1.0 + 0.9 * rng.uniform(size=(n_star, 3))))
            anc = np.repeat(anc, 6, axis=0)[:t0.size]
            a32, s32, found = _reject(rng, self.bx, A, t0, 0, anchors=anc.astype(np.float32).astype(np.float64))
            assert found.all(), f"{cell} {rname}: {int((~found).sum())} intended distances of frame 0 were not found"
            pos0 = np.concatenate([a32[::6], s32]).astype(np.float64)
            self.i0, self.j0 = np.arange(t0.size) // 6, n_star + np.arange(t0.size)
        else:
            pos0, self.i0, self.j0 = _lines(t0, float(np.diag(A).min()))
        self.t0 = t0
        N = pos0.shape[0]
        # ---- frame 1
        e = edges(self.rmin, self.rmax)
        e = np.unique(e[e >= f32(2.0 ** -40)])
        npairs, self.n_edge = N // 2, int(e.size)
        assert npairs >= e.size + 64
        a1, s1, found = _reject(rng, self.bx, A, e, TOL1)
        assert found.all(), f"{cell} {rname}: {int((~found).sum())} edges have no pair in frame 1"
        te = np.resize(e[e >= f32(0.25 * self.rmax)], npairs - e.size)
        a2, s2, f2 = _reject(rng, self.bx, A, te, TOL1, face=True, rounds=6)
        a2[~f2] = (rng.uniform(0.0, 1.0, (int((~f2).sum()), 3)) @ A.T).astype(np.float32)      # nothing found: two atoms somewhere
        s2[~f2] = (rng.uniform(0.0, 1.0, (int((~f2).sum()), 3)) @ A.T).astype(np.float32)
        pos1 = np.concatenate([a1, a2, s1, s2, np.zeros((N - 2 * npairs, 3), np.float32)])
        self.i1, self.j1 = np.arange(npairs), npairs + np.arange(npairs)
        self.t1, self.face1 = np.concatenate([e, te]), np.concatenate([np.zeros(e.size, bool), f2])
        self.coords = np.ascontiguousarray(np.stack([pos0.astype(np.float32).T, pos1.T]))
        self.N = N
        self.all = np.arange(N, dtype=np.int32)
        self._d, self._want = {}, {}

    def distances(self, f):
        """every ordered pair of frame f up to r_max, once"""
        if f not in self._d:
            self._d[f] = R.distances(self.coords[f], self.bx, self.all, self.all, self.rmax)
        return self._d[f]

    def want(self, closed):
        """-> (counts of frame 0, counts of both frames) by the fp32 tier"""
        if closed not in self._want:
            h = [R.histogram(self.distances(f), self.rmin, self.rmax, closed) for f in (0, 1)]
            self._want[closed] = (h[0], h[0] + h[1])
        return self._want[closed]


_SYSTEMS = {}


def system(cell, rname):
    if (cell, rname) not in _SYSTEMS:
        _SYSTEMS[(cell, rname)] = System(cell, rname)
    return _SYSTEMS[(cell, rname)]


def coverage(sy):
    """the conditions of the module's head, from the reference alone; -> dict of the printed figures"""
    what = f"{sy.cell} {sy.rname}"
    assert sy.N <= 4200, (what, sy.N)
    d0 = R.pair_distance(sy.coords[0], sy.bx, sy.i0, sy.j0)
    np.testing.assert_array_equal(d0.view(np.uint32), sy.t0.view(np.uint32), err_msg=f"{what}: frame 0 does not hold the intended distances")
    e = edges(sy.rmin, sy.rmax)
    have = set(d0.view(np.uint32).tolist())
    for k in (-1, 0, 1):
        assert set(step(e[1:-1], k).view(np.uint32).tolist()) <= have, f"{what}: an inner edge has no pair {k:+d} floats from it"
    for k in range(-3, 4):
        ends = step(e[[0, -1]], k)
        assert set(ends[ends >= f32(2.0 ** -40)].view(np.uint32).tolist()) <= have, f"{what}: r_min / r_max has no pair {k:+d} floats from it"
    assert f32(sy.rmax) in d0 and (sy.rmin == 0.0 or f32(sy.rmin) in d0)
    d1 = R.pair_distance(sy.coords[1], sy.bx, sy.i1, sy.j1)
    apart = np.abs(floats_apart(d1, sy.t1))
    assert (apart[:sy.n_edge] <= TOL1).all() and (apart[sy.face1] <= TOL1).all(), f"{what}: frame 1 left its edges"
    inner = np.unique(e[1:-1][e[1:-1] >= f32(2.0 ** -40)])
    d1s = np.sort(d1)
    at = np.clip(np.searchsorted(d1s, inner), 1, d1s.size - 1)
    nearest = np.minimum(np.abs(floats_apart(d1s[at], inner)), np.abs(floats_apart(d1s[at - 1], inner)))
    assert (nearest <= TOL1).all(), f"{what}: an inner edge has no pair of frame 1 within {TOL1} floats"
    A = _cell_matrix(sy.box)
    crossing = _crosses(sy.bx, A, sy.coords[1][:, sy.i1].T, sy.coords[1][:, sy.j1].T) & (apart <= TOL1)
    assert int(crossing.sum()) >= 16, f"{what}: only {int(crossing.sum())} pairs of frame 1 cross a periodic face"
    assert int((crossing & sy.face1).sum()) == int(sy.face1.sum())
    delta = float(R.fast_delta(sy.rmin, sy.rmax))
    assert (delta < 0.25) == sy.fast, f"{what}: delta = {delta}"
    fig = dict(N=sy.N, delta=delta, crossing=int(crossing.sum()))
    for f in (0, 1):
        d = sy.distances(f)
        d = d[(d >= f32(sy.rmin)) & (d <= f32(sy.rmax))]
        fig[f"parked{f}"] = int((R.offsets(d, sy.rmin, sy.rmax) < delta).sum()) if sy.fast else int(d.size)
        c = R.compare(d, sy.rmin, sy.rmax, closed=True, what=f"{what} frame {f}")
        fig[f"hits{f}"], fig[f"near{f}"], fig[f"differ{f}"], fig[f"worst{f}"] = c["hits"], c["near"], c["differ"], c["worst"]
    print(f"bin_edges {what}: N = {sy.N}, delta = {delta:.4g}, frame 1: {fig['crossing']} of {d1.size} pairs across a face; "
          f"ordered pairs in [r_min, r_max] / parked / within the exact margin / fp32 bin != exact bin (worst offset "
          f"over margin): frame 0 {fig['hits0']} / {fig['parked0']} / {fig['near0']} / {fig['differ0']} ({fig['worst0']:.3f}), "
          f"frame 1 {fig['hits1']} / {fig['parked1']} / {fig['near1']} / {fig['differ1']} ({fig['worst1']:.3f})")
    return fig


def against_oracle(O, sy):
    """the fp32 tier and the oracle's all-pairs evaluation, bit for bit, open and closed, frame by frame"""
    ocell, _ = cases.cell_pair(O, sy.box, 7)
    for closed in (0, 1):
        old = O.set_spec("rdf_closed", closed)
        try:
            for f in (0, 1):
                got, _ = O.rdf_frame(sy.coords[f, 0], sy.coords[f, 1], sy.coords[f, 2], ocell, sy.all, sy.all, sy.rmin, sy.rmax, method="brute")
                np.testing.assert_array_equal(got, R.histogram(sy.distances(f), sy.rmin, sy.rmax, bool(closed)),
                                              err_msg=f"{sy.cell} {sy.rname}: frame {f}, closed = {closed}: the oracle and tests/rdf_ref.py differ")
        finally:
            O.set_spec("rdf_closed", old)


# ---- the routes -------------------------------------------------------------------------------------------------------------------------

# name -> (cell, options, kernel family, shell)
ROUTES = {
    "pencil_v0_pop0_shared": ("cube_39", dict(rdf_variant=0, rdf_pop=0, rdf_shared_hist=1), "pencil", False),
    "pencil_v0_pop1_shared": ("cube_39", dict(rdf_variant=0, rdf_pop=1, rdf_shared_hist=1), "pencil", False),
    "pencil_v0_pop0_per_wave": ("cube_39", dict(rdf_variant=0, rdf_pop=0, rdf_shared_hist=0), "pencil", False),
    "pencil_v0_pop1_per_wave": ("cube_39", dict(rdf_variant=0, rdf_pop=1, rdf_shared_hist=0), "pencil", False),
    "pencil_v1": ("cube_39", dict(rdf_variant=1), "pencil", False),
    "pencil_v2": ("cube_39", dict(rdf_variant=2), "pencil", False),
    "pencil_v3": ("cube_39", dict(rdf_variant=3), "pencil", False),
    "pencil_triclinic_v0": ("triclinic", dict(rdf_variant=0), "pencil", False),
    "pencil_triclinic_v2": ("triclinic", dict(rdf_variant=2), "pencil", False),
    "brute": ("small", dict(), "brute", False),
    "brute_masked": ("small", dict(), "brute", True),
}


def folded_pop(rname):
    """rdf_pop = 1 differs from 0 only where the folded test applies: r_min == 0 and a usable fast path (p.pop of the launch)"""
    rmin, _, fast = RANGES[rname]
    return fast and rmin == 0.0


# the rdf_pop = 1 routes run where they are a kernel of their own; elsewhere they would repeat the rdf_pop = 0 case instruction for instruction
PARAMS = [(route, rname) for route in ROUTES for rname in RANGES if "pop1" not in route or folded_pop(rname)]


def _frames(lib, sy, shell, device):
    """-> (counts after frame 0, counts after frame 1)"""
    ir = V.ScriptIR(lib)
    if shell:
        ir.add_rdf_shell("g", sy.all, sy.all, (sy.rmin, sy.rmax), target_shell=(sy.all, 0.0, 1.0))      # d = 0 with itself: every atom stays
    else:
        ir.add_rdf("g", sy.all, sy.all, (sy.rmin, sy.rmax))
    vcell = V.make_unitcell(*_unitcell_args(sy.box))
    ev = V.ScriptEval(2, ir)
    traj = cases.make_traj(lib, sy.coords, vcell, device)
    sysm = V.MolSystem(sy.N, unitcell=vcell)
    out = []
    for f in (0, 1):
        assert ev.frame_range(sysm, traj, f, f + 1)
        out.append(np.array(ev.property_data("g").counts, copy=True))
    assert ev.frame_mask().all()
    return out


def _unitcell_args(box):
    if np.isscalar(box):
        return box, 7, (0.0, 0.0, 0.0)
    return tuple(box[:3]), 7, tuple(box[3:])


def run(lib, rname, route, device=False):
    cell, opts, family, shell = ROUTES[route]
    sy = system(cell, rname)
    for closed in (0, 1):
        lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
        try:
            with options(lib, spec_rdf_closed=closed, **opts):          # restores every switch on the way out
                got = _frames(lib, sy, shell, device)
        finally:
            lib.vmd_profile_enable(False)
        n_grid, n_brute = cases._kernel_family(lib)
        assert (n_grid > 0 and n_brute == 0) if family == "pencil" else (n_brute > 0 and n_grid == 0), \
            f"{route} {rname}: {n_grid} pencil and {n_brute} all-pairs launches"
        want = sy.want(bool(closed))
        for f in (0, 1):
            np.testing.assert_array_equal(got[f], want[f], err_msg=f"{route} {rname}: closed = {closed}, after frame {f}: counts differ from tests/rdf_ref.py")
    # the pairs exactly at r_min / r_max: out of the open interval, in the closed one.  From the reference: the two differ by those alone
    d = np.concatenate([sy.distances(0), sy.distances(1)])
    at_ends = int((d == f32(sy.rmax)).sum()) + int((d == f32(sy.rmin)).sum())
    assert at_ends > 0 and int(sy.want(True)[1].sum()) - int(sy.want(False)[1].sum()) == at_ends
