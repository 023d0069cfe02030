"""Solvent-accessible surface area on the emulator build and in the host-only entry points.  The rule is EXACT EQUALITY with
the numpy restatement (tests/sasa_ref.py) for every output - the point counts of a frame, every accumulator of the record, the u64 totals
and the temporal floats - and every launch choice (walk or all pairs, batch size, call pattern) bit-identical to the others.  Every check
prints how many candidate pairs lie within 4 ulp of s * s and how many point tests within 4 ulp of t_ij, so that a reader sees the equality
was exercised.  Scenarios: known answers (one atom, an atom inside a larger one, two equal spheres against the analytic cap, an interface
area); a hand-placed pair across the faces, an edge and a corner of a cell, tilted and with an open axis; the size edges of both lists and
of the point mask, in a roomy cell, in one just large enough for a grid and in one too small; planted thresholds under both
spec_within_closed settings and mixed radii; identity and coincidence; the call patterns; a batch repeated for a bucket overflow; the
two-rank merge; the radii helper; and the IR cases - every refusal, the fingerprint field by field, the statement next to the default script
and the other forms.  tests/test_sasa_gpu.py runs the same scenario functions on the device."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import viamd_amd as V
from viamd_amd import _lib as L
from viamd_amd import script

import cases
import hbond_cases as HC
import sasa_cases as SC
import sasa_ref as R
import test_geometry as TG
import test_rmsd as TR
from test_hbond import Options, ref_box, steps
from test_rama import OPT_INS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("area", "pts")
WALK, BRUTE = dict(shell_brute_below=0), dict(shell_brute_below=1 << 30)
ROUTES = (dict(), WALK, BRUTE)
NEAR = {}                        # what -> (candidate pairs near s * s, point tests near t_ij), as printed
# DESIGN 1.15, "two equal spheres": the largest deviation of the restatement's accessible fraction at P = 256 from (1 + d / 2R) / 2 over
# CAP_D, as measured there (0.00795, two points of 256); the test allows twice that
CAP_D = (0.5, 1.0, 1.7, 2.3, 3.1, 4.0, 5.0, 5.7)
CAP_DEVIATION = 0.0080

_points = {}


def points_of(lib, P):
    """the library's table (vmd_sasa_points): what the kernels read and what the restatement takes"""
    if P not in _points:
        _points[P] = script.sasa_points(P, lib=lib)
    return _points[P]


def sasa_ir(lib, lists, probe=SC.PROBE, npoints=SC.NPOINTS, names=NAMES):
    ir = V.ScriptIR(lib)
    ir.add_sasa_lists(names, lists["measured"], lists["measured_radius"], lists["env"], lists["env_radius"], probe, npoints)
    return ir


class Run:
    """one evaluation: the eval and what a single-frame query needs"""

    def __init__(self, lib, ir, coords, cell, device=False, ranges=None, pooled=None):
        box, tilt, flags = cell
        F, _, N = coords.shape
        self.cell = V.make_unitcell(box, flags, tilt)
        self.ev = V.ScriptEval(F, ir)
        self.sysm = V.MolSystem(N, unitcell=self.cell)
        self.traj = cases.make_traj(lib, coords, self.cell, device)
        for beg, end in ([(0, F)] if ranges is None else ranges):
            assert (self.ev.frame_range_pooled(self.sysm, self.traj, beg, end, *pooled) if pooled else
                    self.ev.frame_range(self.sysm, self.traj, beg, end))

    def area(self, name=NAMES[0]):
        return TG.rows(self.ev, name)[:, 0]

    def record(self, name=NAMES[1]):
        return self.ev.property_data(name).sasa_accumulators.copy()

    def atoms(self, frame, name=NAMES[0]):
        return self.ev.sasa_atoms(name, self.sysm, self.traj, frame)


def run(lib, lists, coords, cell, device=False, probe=SC.PROBE, npoints=SC.NPOINTS, **kw):
    return Run(lib, sasa_ir(lib, lists, probe, npoints), coords, cell, device, **kw)


def restate(lib, coords, cell, lists, probe=SC.PROBE, npoints=SC.NPOINTS, closed=False, frames=None):
    bx, flags = ref_box(cell)
    return R.evaluate(coords, bx, lists["measured"], lists["measured_radius"], lists["env"], lists["env_radius"], probe, points_of(lib, npoints),
                      closed=closed, flags=flags, frames=frames)


def check(rn, want, lists, what, probe=SC.PROBE, npoints=SC.NPOINTS, list_frames=None):
    """every output against the restatement `want`, exactly, and the invariants of every scenario"""
    nmeas = len(lists["measured"])
    got_a, got_r = rn.area(), rn.record()
    NEAR[what] = (want["near_s"], want["near_t"])
    frames = sorted(want["counts"])
    print(f"{what}: {int(want['record'][:-1].sum())} accessible points in {int(want['record'][-1])} frames, {want['neighbours']} neighbours, "
          f"{want['near_s']} candidate pairs within 4 ulp of s * s, {want['near_t']} point tests within 4 ulp of t_ij")
    assert got_a.dtype == np.float32 and np.array_equal(got_a.view(np.int32), want["area"].view(np.int32)), what
    assert got_r.shape == (nmeas + 1,) and np.array_equal(got_r, want["record"]), what
    assert (got_r[:-1] <= np.uint64(npoints) * got_r[-1]).all(), what
    # the reader: count / frames * 4 pi R^2 / P in double
    mean, F = rn.ev.sasa(NAMES[1])
    assert F == int(got_r[-1])
    Rm = R.big_r(lists["measured_radius"], probe).astype(np.float64)
    ref_mean = got_r[:-1].astype(np.float64) / max(F, 1) * (4.0 * math.pi * Rm * Rm) / npoints if F else np.zeros(nmeas)
    assert np.allclose(mean, ref_mean, rtol=1e-14, atol=0.0), what
    # the u64 totals: the temporal float is (float)(total * 2^-20), and the totals are the counts times the weights
    w = R.weights(R.big_r(lists["measured_radius"], probe), npoints)
    for f in (frames if list_frames is None else list_frames):
        got = rn.atoms(f)
        assert got.dtype == np.uint32 and np.array_equal(got, want["counts"][f]), (what, f)
        total = sum(int(c) * wi for c, wi in zip(got, w))
        assert total == want["totals"][f] and got_a[f] == np.float32(np.float64(total) * 2.0 ** -20), (what, f)
    return got_a, got_r


def same(a, b, what):
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1]), what


def all_routes(lib, lists, coords, cell, want, what, device=False, probe=SC.PROBE, npoints=SC.NPOINTS, list_frames=None, **opts):
    one = None
    for route in ROUTES:
        with Options(lib, **dict(opts, **route)):
            got = check(run(lib, lists, coords, cell, device, probe, npoints), want, lists, f"{what}, {route}", probe, npoints, list_frames)
        one = one or got
        same(got, one, (what, route))
    return one


def lists_of(atoms, radii, measured=None):
    a, r = np.asarray(atoms, np.int32), np.asarray(radii, np.float32)
    m = np.arange(a.size) if measured is None else np.asarray(measured)
    return dict(measured=a[m], measured_radius=r[m], env=a, env_radius=r)


ROOMY = ((30.0, 30.0, 30.0), (0.0, 0.0, 0.0), 7)


# ---- 1. known answers -------------------------------------------------------------------------------------------------------------------------

def known_answers(lib, device=False):
    P = 96
    # one atom alone: n = P, total = P * w
    coords = np.array([[[7.0], [8.0], [9.0]]], np.float32)
    lists = lists_of([0], [1.7])
    want = restate(lib, coords, ROOMY, lists, npoints=P)
    w = R.weights(R.big_r([1.7], SC.PROBE), P)[0]
    assert list(want["counts"][0]) == [P] and want["totals"][0] == P * w
    assert abs(want["area"][0] - 4.0 * math.pi * 3.1 ** 2) < 1e-3
    got = all_routes(lib, lists, coords, ROOMY, want, "one atom alone", device, npoints=P)
    assert list(got[1]) == [P, 1]
    # an atom inside a larger one: no point of it is accessible; the larger one keeps all of its points
    coords = np.array([[[7.0, 7.25], [8.0, 8.0], [9.0, 9.0]]], np.float32)
    lists = lists_of([0, 1], [1.0, 3.0])
    want = restate(lib, coords, ROOMY, lists, npoints=P)
    assert list(want["counts"][0]) == [0, P]
    all_routes(lib, lists, coords, ROOMY, want, "an atom inside a larger one", device, npoints=P)


def test_known_answers_on_the_emulator(emu_lib):
    known_answers(emu_lib)


def two_spheres(lib, device=False):
    """Two equal spheres of radius R at distance d: the accessible fraction of either is (1 + d / 2R) / 2.  The RESTATEMENT is held to the
    analytic value at P = 256 (twice the deviation DESIGN 1.15 records), the library to the restatement exactly."""
    P, rad = 256, 1.5
    Rr = float(np.float32(rad) + np.float32(SC.PROBE))
    coords = np.stack([np.array([[5.0, 5.0 + d], [6.0, 6.0], [7.0, 7.0]], np.float32) for d in CAP_D])
    lists = lists_of([0, 1], [rad, rad])
    want = restate(lib, coords, ROOMY, lists, npoints=P)
    worst = 0.0
    for f, d in enumerate(CAP_D):
        d32 = float(coords[f, 0, 1] - coords[f, 0, 0])
        for n in want["counts"][f]:
            worst = max(worst, abs(n / P - 0.5 * (1.0 + d32 / (2.0 * Rr))))
    print(f"two equal spheres, P = {P}: largest deviation of the restatement from (1 + d / 2R) / 2 over d = {CAP_D}: {worst:.5f}")
    assert worst <= 2.0 * CAP_DEVIATION
    all_routes(lib, lists, coords, ROOMY, want, "two equal spheres", device, npoints=P)


def test_two_equal_spheres_on_the_emulator(emu_lib):
    two_spheres(emu_lib)


def interface_area(lib, device=False):
    """SASA(A) + SASA(B) - SASA(AB) >= 0 for two touching groups (the halves of a water droplet): another occluder only clears more bits, so
    it holds entry by entry in the integers, and for the areas"""
    n_w = 120
    coords = HC.water_box(n_w, (12.0, 12.0, 12.0), 2, seed=21, spread=1.0)
    cell = ((60.0, 60.0, 60.0), (0.0, 0.0, 0.0), 7)
    rad = SC.water_radii(n_w)
    left = np.nonzero(np.repeat(coords[0, 0, 0::3] < 6.0, 3))[0].astype(np.int32)
    right = np.setdiff1d(np.arange(3 * n_w, dtype=np.int32), left)
    assert left.size > 60 and right.size > 60
    ir = V.ScriptIR(lib)
    both = np.concatenate([left, right])
    for nm, atoms in (("a", left), ("b", right), ("ab", both)):
        ir.add_sasa((nm, nm + "_pts"), atoms, rad[atoms])
    rn = Run(lib, ir, coords, cell, device)
    a, b, ab = (rn.area(k) for k in ("a", "b", "ab"))
    print(f"interface area per frame: {a + b - ab} A^2 of {a}, {b}")
    assert (a + b - ab > 1.0).all()
    for f in range(2):
        sep = np.concatenate([rn.atoms(f, "a"), rn.atoms(f, "b")])
        assert (sep >= rn.atoms(f, "ab")).all()
    for nm, atoms in (("a", left), ("ab", both)):
        want = restate(lib, coords, cell, lists_of(atoms, rad[atoms]))
        assert np.array_equal(rn.area(nm).view(np.int32), want["area"].view(np.int32))
        assert np.array_equal(rn.record(nm + "_pts"), want["record"])


def test_interface_area_on_the_emulator(emu_lib):
    interface_area(emu_lib)


def hand_placed_pairs(lib, device=False):
    """Two atoms 2.5 A apart: each buries part of the other.  Frame by frame the pair is moved so that it crosses each face, an edge and a
    corner of a cubic cell; then the same in a tilted cell, and with the x axis open (where a pair across the open face is no pair: both
    atoms are fully exposed)."""
    P = 96
    rng = np.random.default_rng(2)
    L_ = 20.0
    spots = [(10.0, 10.0, 10.0), (L_ - 1.0, 10.0, 10.0), (10.0, L_ - 1.0, 10.0), (10.0, 10.0, L_ - 1.0), (L_ - 1.0, L_ - 0.5, 10.0),
             (L_ - 0.5, L_ - 0.5, L_ - 0.5), (-1.0, 3.0 * L_ + 0.5, -L_ - 1.0)]
    axes = [np.eye(3), np.eye(3), np.eye(3)[[1, 0, 2]], np.eye(3)[[2, 1, 0]]]          # the pair along x, x, y, z: across the face it stands at
    frames = []
    for k, sp in enumerate(spots):
        rot = axes[k] if k < 4 else HC.rotation(rng)
        frames.append((np.array([[0.0, 0.0, 0.0], [2.5, 0.0, 0.0]]) @ rot.T + np.asarray(sp)).T)
    coords = np.stack(frames).astype(np.float32)
    lists = lists_of([0, 1], [1.5, 2.0])
    for cell in (((L_, L_, L_), (0.0, 0.0, 0.0), 7), ((L_, L_, L_), (4.0, -2.0, 3.0), 7)):
        want = restate(lib, coords, cell, lists, npoints=P)
        for f in range(len(spots)):
            assert (want["counts"][f] > 0).all() and (want["counts"][f] < P).all(), (cell, f)
        all_routes(lib, lists, coords, cell, want, f"pair, tilt {cell[1]}", device, npoints=P)
    # the same pairs folded into the cubic cell by hand: with every axis periodic nothing changes; with x open the pair that stood across
    # the x face is 17.5 A apart, and both atoms are fully exposed
    folded = coords.copy()
    folded[:6] = np.mod(folded[:6], np.float32(L_))
    want = restate(lib, folded, ((L_, L_, L_), (0.0, 0.0, 0.0), 7), lists, npoints=P)
    for f in range(4):
        assert (want["counts"][f] > 0).all() and (want["counts"][f] < P).all(), f
    cell =((L_, L_, L_), (0.0, 0.0, 0.0), 6)
    want = restate(lib, folded, cell, lists, npoints=P)
    assert list(want["counts"][1]) == [P, P] and (want["counts"][0] < P).all() and (want["counts"][2] < P).all() and (want["counts"][3] < P).all()
    all_routes(lib, lists, folded, cell, want, "pair, x open", device, npoints=P)


def test_hand_placed_pairs_on_the_emulator(emu_lib):
    hand_placed_pairs(emu_lib)


# ---- 2. size edges ----------------------------------------------------------------------------------------------------------------------------

N_W = 500


def size_sweep(lib, ci, device=False):
    """nmeas x nenv of sasa_cases in cell ci: the default route (all pairs below 480 environment entries, the walk from there), the walk and
    all pairs forced through shell_brute_below, each with batch_frames 1 and 2 - one answer"""
    cell = SC.CELLS[ci]
    coords = HC.water_box(N_W, cell[0], 2, seed=3 + ci)
    for nmeas in SC.NMEAS:
        for nenv in SC.NENV:
            lists = SC.subset_lists(N_W, nmeas, nenv, seed=100 * ci + nmeas + nenv)
            want = restate(lib, coords, cell, lists)
            what = f"cell {ci}, {nmeas} measured x {nenv} environment"
            one = None
            for route in ROUTES:
                for bf in (1, 2):
                    with Options(lib, batch_frames=bf, **route):
                        rn = run(lib, lists, coords, cell, device)
                        if one is None:
                            one = check(rn, want, lists, what, list_frames=[1])
                        else:
                            same((rn.area(), rn.record()), one, (what, route, bf))
            if device and nmeas == 257 and nenv == 481:
                rn = run(lib, lists, coords, cell)
                same((rn.area(), rn.record()), one, (what, "host-staged"))


@pytest.mark.parametrize("ci", range(len(SC.CELLS)))
def test_size_edges_on_the_emulator(emu_lib, ci):
    size_sweep(emu_lib, ci)


def npoints_edges(lib, device=False):
    """the word seams of the point mask, walk and all pairs"""
    cell = SC.CELLS[0]
    n_w = 200
    coords = HC.water_box(n_w, cell[0], 2, seed=17)
    lists = SC.subset_lists(n_w, 130, 3 * n_w, seed=5)
    for P in SC.NPOINTS_EDGES:
        want = restate(lib, coords, cell, lists, npoints=P)
        assert 0 < want["record"][:-1].sum() < 2 * 130 * P or P == 1
        one = None
        for route in (WALK, BRUTE):
            with Options(lib, **route):
                got = check(run(lib, lists, coords, cell, device, npoints=P), want, lists, f"{P} points, {route}", npoints=P, list_frames=[0])
            one = one or got
            same(got, one, (P, route))


def test_npoints_edges_on_the_emulator(emu_lib):
    npoints_edges(emu_lib)


def test_points_table(host_lib):
    """vmd_sasa_points against the numpy statement of D-SASA-POINTS: within 1 fp32 ulp per component; unit vectors; the refusals"""
    for P in SC.NPOINTS_EDGES + [2, 7]:
        got = script.sasa_points(P, lib=host_lib)
        ref = R.points_formula(P)
        assert got.shape == (P, 3) and got.dtype == np.float32
        # (a component next to zero is held absolutely: one ulp of 1 there)
        ok = (R.ulps_between(got, ref) <= 1) | (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= 2.0 ** -24)
        assert ok.all(), P
        assert np.allclose((got.astype(np.float64) ** 2).sum(axis=1), 1.0, atol=3e-7)
    for P in (0, 257, 1 << 20):
        with pytest.raises(script.ScriptError, match=r"\[1, 256\]"):
            script.sasa_points(P, lib=host_lib)
    assert host_lib.vmd_sasa_points(4, None, 0) == 4                         # count only
    assert host_lib.vmd_sasa_points(4, None, 2) == 0 and "NULL" in host_lib.last_error()


def tight_boxes(lib, device=False):
    """A cell just large enough for a grid at r_cut (two pencils per axis: every neighbour pencil is met under two images) and one too
    small, where the walk cannot be had and all pairs answer whatever is asked"""
    for edge, grid in ((SC.TIGHT, True), (SC.TOO_SMALL, False)):
        cell = ((edge, edge, edge), (0.0, 0.0, 0.0), 7)
        n_w = 55
        coords = HC.water_box(n_w, cell[0], 2, seed=11)
        lists = SC.water_lists(n_w)
        want = restate(lib, coords, cell, lists)
        one = None
        for route in ROUTES:
            lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
            try:
                with Options(lib, **route):
                    got = check(run(lib, lists, coords, cell, device), want, lists, f"edge {edge}, {route}", list_frames=[0])
            finally:
                lib.vmd_profile_enable(False)
            n = C.c_uint64(0)
            lib.vmd_profile_ms(b"sasa_atoms", C.byref(n))
            assert (n.value > 0) == (grid and route is WALK), (edge, route, n.value)
            one = one or got
            same(got, one, (edge, route))


def test_tight_boxes_on_the_emulator(emu_lib):
    tight_boxes(emu_lib)


# ---- 3. thresholds ----------------------------------------------------------------------------------------------------------------------------

def planted_thresholds(r_i, r_j):
    """Two atoms per FRAME on the x axis at s = R_i + R_j moved by -4 .. 4 ulp, from two positions of the first: rule 2 decides whether the
    second is a neighbour at all.  Then the second at a distance where its sphere cuts the first's through the ring of points around
    z = u_kz for a few k, moved by -4 .. 4 ulp: rule D-SASA-POINT decides for the points next to the cut."""
    Ri, Rj = (np.float32(r) + np.float32(SC.PROBE) for r in (r_i, r_j))
    s = np.float32(Ri + Rj)
    frames = []
    for dx in steps(s, -4, 4):
        for base in (5.0, 4.0 + 1.0 / 3.0):
            frames.append([(base, 2.0, 5.0), (float(np.float32(base) + dx), 2.0, 5.0)])
    pts = R.points_formula(SC.NPOINTS).astype(np.float64)
    for k in (3, 40, 77):
        # the neighbour along -z at distance d buries point k iff u_kz * d < t(d): t(d) = u_kz d solved for d in float64, then stepped
        c = -pts[k, 2]
        a, b, cc = 1.0, 2.0 * float(Ri) * c, float(Ri) ** 2 - float(Rj) ** 2         # d^2 + 2 R_i c d + R_i^2 - R_j^2 = 0
        disc = b * b - 4 * a * cc
        if disc <= 0:
            continue
        d = (-b + math.sqrt(disc)) / 2.0
        if not (0.2 < d < float(s)):
            continue
        for dz in steps(np.float32(d), -4, 4):
            frames.append([(5.0, 2.0, 5.0), (5.0, 2.0, float(np.float32(5.0) + dz))])
    coords = np.asarray(frames, np.float64).transpose(0, 2, 1).astype(np.float32)
    return coords, lists_of([0, 1], [r_i, r_j])


def thresholds(lib, device=False):
    cell = ((40.0, 40.0, 40.0), (0.0, 0.0, 0.0), 7)
    for r_i, r_j in ((1.5, 1.5), (1.2, 1.9), (2.0, 1.0)):
        coords, lists = planted_thresholds(r_i, r_j)
        for closed in (0, 1):
            want = restate(lib, coords, cell, lists, closed=bool(closed))
            # (2 ulp of s are 3 ulp of s * s: the planted steps -2 .. 2 lie within 4 ulp; with equal radii s is r_cut, and only the steps
            # below it are candidates at all)
            assert want["near_s"] >= 4, (r_i, r_j, want["near_s"])
            one = None
            for route in (WALK, BRUTE):
                with Options(lib, spec_within_closed=closed, **route):
                    got = check(run(lib, lists, coords, cell, device), want, lists, f"thresholds, radii {r_i} / {r_j}, closed {closed}, {route}")
                one = one or got
                same(got, one, (r_i, r_j, closed, route))
    assert any(NEAR[k][1] > 0 for k in NEAR if k.startswith("thresholds"))


def test_thresholds_on_the_emulator(emu_lib):
    thresholds(emu_lib)


def mixed_radii(lib, device=False):
    """one fat environment atom in a hundred: r_cut = 14.8 A is far from the tight bound of most pairs, rule 2 does the work.  The answer
    must not depend on how tight r_cut is: the water box's own entries answer as they do without the fat atoms' cutoff"""
    n_w = 400
    cell = ((32.0, 32.0, 32.0), (0.0, 0.0, 0.0), 7)
    coords = HC.water_box(n_w, cell[0], 2, seed=23)
    lists = SC.mixed_radii_lists(n_w, seed=2)
    want = restate(lib, coords, cell, lists)
    all_routes(lib, lists, coords, cell, want, "mixed radii", device, list_frames=[0])


def test_mixed_radii_on_the_emulator(emu_lib):
    mixed_radii(emu_lib)


def water_box_near(lib):
    """the water box cases must show a non-zero number of candidate pairs near s * s and of point tests near t_ij"""
    # (a pair lands within 4 ulp of s * s about once in a million candidates: the box is packed - 1 200 atoms in 14 A, most of them
    # candidates of each other - so that four frames hold a few)
    cell = ((14.0, 14.0, 14.0), (0.0, 0.0, 0.0), 7)
    n_w = 400
    coords = HC.water_box(n_w, cell[0], 4, seed=29)
    lists = SC.water_lists(n_w)
    want = restate(lib, coords, cell, lists)
    all_routes(lib, lists, coords, cell, want, "water box, every atom against every atom", list_frames=[2])
    assert want["near_s"] > 0 and want["near_t"] > 0, (want["near_s"], want["near_t"])


def test_water_box_meets_the_thresholds(emu_lib):
    water_box_near(emu_lib)


# ---- 4. identity and coincidence --------------------------------------------------------------------------------------------------------------

def identity(lib, device=False):
    cell = SC.CELLS[0]
    n_w = 300
    coords = HC.water_box(n_w, cell[0], 2, seed=5).copy()
    rad = SC.water_radii(n_w)
    N = 3 * n_w
    every = np.arange(N, dtype=np.int32)
    # measured atoms that are not in the environment (the hydrogens against the oxygens), and an environment that is a strict superset
    for what, lists in (("measured not in env", dict(measured=every[1::3], measured_radius=rad[1::3], env=every[0::3], env_radius=rad[0::3])),
                        ("env a strict superset", lists_of(every, rad, measured=np.arange(0, N, 7)))):
        want = restate(lib, coords, cell, lists)
        all_routes(lib, lists, coords, cell, want, what, device, list_frames=[1])
    # an atom listed twice on both sides: the two measured entries answer alike, the second environment entry changes nothing
    twice = lists_of(np.concatenate([every, [6, 6]]), np.concatenate([rad, rad[[6, 6]]]), measured=np.concatenate([[6, N, N + 1], np.arange(30, 90)]))
    want = restate(lib, coords, cell, twice)
    got = all_routes(lib, twice, coords, cell, want, "an atom listed twice", device, list_frames=[0])
    assert got[1][0] == got[1][1] == got[1][2]
    # two atoms of different radius on one point, bit for bit: D-SASA-COINCIDENT, the lowest environment entry answers for both - with ITS
    # atom and ITS radius.  b is listed in front of a and carries the larger radius
    a, b = 30, 333
    c2 = coords.copy()
    c2[:, :, b] = c2[:, :, a]
    r2 = rad.copy()
    r2[b] = 2.4
    order = np.concatenate([[b], np.delete(every, b)])
    co = lists_of(order, r2[order], measured=np.concatenate([np.nonzero(order == a)[0], [0], np.arange(40, 200)]))
    want = restate(lib, c2, cell, co)
    assert want["counts"][0][0] == 0                        # a lies at the centre of the larger b: nothing of it is accessible
    all_routes(lib, co, c2, cell, want, "two atoms on one point", device, list_frames=[0, 1])
    # measured atoms far outside the cell: whole cells (a million of them) move nothing
    far = coords.copy()
    far[:, 0, 0:90] += np.float32(cell[0][0]) * np.float32(1.0e6)
    lists = lists_of(every, rad, measured=np.arange(0, 150))
    want = restate(lib, far, cell, lists)
    all_routes(lib, lists, far, cell, want, "a million cells away", device, list_frames=[0])


def test_identity_on_the_emulator(emu_lib):
    identity(emu_lib)


# ---- 5. call patterns -------------------------------------------------------------------------------------------------------------------------

def call_patterns(lib, device=False):
    """one call; many small ranges in shuffled order; pool threads; clear_data then again; a frame evaluated twice counts twice; a partial
    range (frames never evaluated read +0 and are not counted); a source's frame blocks"""
    cell = SC.CELLS[0]
    n_w, F = 200, 8
    coords = HC.water_box(n_w, cell[0], F, seed=9)
    lists = SC.water_lists(n_w)
    want = restate(lib, coords, cell, lists)
    with Options(lib, **WALK):
        first = run(lib, lists, coords, cell, device)
        one = check(first, want, lists, "one call", list_frames=[0, F - 1])
        order = [(f, f + 1) for f in np.random.default_rng(4).permutation(F)]
        for kw in (dict(ranges=[(5, 8), (0, 2), (2, 5)]), dict(ranges=order), dict(pooled=(16, 1)), dict(pooled=(4, 2))):
            rn = run(lib, lists, coords, cell, device, **kw)
            same((rn.area(), rn.record()), one, kw)
        with Options(lib, batch_frames=3):
            rn = run(lib, lists, coords, cell, device)
            same((rn.area(), rn.record()), one, "batch_frames 3")
        # the single-frame query touches nothing accumulated
        before = first.record()
        first.atoms(3)
        assert np.array_equal(first.record(), before) and np.array_equal(first.area().view(np.int32), one[0].view(np.int32))
        first.ev.clear_data()
        assert not first.record().any() and first.ev.sasa(NAMES[1])[1] == 0 and not first.ev.sasa(NAMES[1])[0].any()
        assert first.ev.frame_range(first.sysm, first.traj, 0, F)
        same((first.area(), first.record()), one, "clear_data, then again")
        # frames 2 .. 4 alone: a partial record, the other rows +0; then the same frames again: counted twice
        part = run(lib, lists, coords, cell, device, ranges=[(2, 5)])
        got = check(part, restate(lib, coords, cell, lists, frames=[2, 3, 4]), lists, "frames 2 .. 4", list_frames=[2])
        assert not got[0][:2].any() and not got[0][5:].any() and got[1][-1] == 3
        assert part.ev.frame_range(part.sysm, part.traj, 2, 5)
        check(part, restate(lib, coords, cell, lists, frames=[2, 3, 4, 2, 3, 4]), lists, "frames 2 .. 4 twice", list_frames=[])
        assert np.array_equal(part.record(), 2 * got[1])
        # a source evaluated in blocks of two frames lends frames 2 .. 3
        ir = sasa_ir(lib, lists)
        src = V.ScriptEval(F, ir)
        src.set_block_frames(2)
        assert src.frame_range(first.sysm, first.traj, 0, F)
        assert np.array_equal(src.property_data(NAMES[1]).sasa_accumulators, one[1])
        flt = V.ScriptEval(F, ir)
        flt.set_block_frames(2)
        flt.set_source(src)
        assert flt.frame_range(first.sysm, first.traj, 2, 4) and flt.frame_stats()[1] > 0
        assert np.array_equal(flt.property_data(NAMES[1]).sasa_accumulators, restate(lib, coords, cell, lists, frames=[2, 3])["record"])


def test_call_patterns_on_the_emulator(emu_lib):
    call_patterns(emu_lib)


def overflow_case(lib, O, device=False):
    """test_hbond.overflow_case's construction: the middle frames pile every oxygen into one pencil, a bucket sized from the batch's ends
    overflows and the batch is repeated.  The record is added to with atomics behind the overflow flag: it must not count that batch twice -
    the record is that of an IR without the rdf, which no overflow ever touches (all pairs)."""
    n, box, F = 3000, 60.0, 12
    coords = cases.water_box(O, 5, n, box, F)
    o = cases.oxygen(n)
    rng = np.random.default_rng(3)
    for f in (5, 6, 7):
        coords[f][:, o] = rng.uniform(1.0, 11.0, (3, o.size)).astype(np.float32)
    rad = np.full(n, SC.R_H, np.float32)
    rad[o] = SC.R_O
    lists = lists_of(np.arange(n, dtype=np.int32), rad, measured=np.arange(0, 300))
    cell = ((box, box, box), (0.0, 0.0, 0.0), 7)
    P = 33
    with Options(lib, **BRUTE):
        alone = run(lib, lists, coords, cell, device, npoints=P)
    one = (alone.area(), alone.record())
    assert one[1][-1] == F and one[1][:-1].any()
    with Options(lib, cells_small=0, cells_cap_sample=2, **WALK):
        for bf in (0, 4):
            with Options(lib, batch_frames=bf):
                ir = sasa_ir(lib, lists, npoints=P)
                ir.add_rdf("goo", o, o, (0.0, 12.0))
                lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
                try:
                    rn = Run(lib, ir, coords, cell, device)
                finally:
                    lib.vmd_profile_enable(False)
                nb = C.c_uint64(0)
                lib.vmd_profile_ms(b"cells_build", C.byref(nb))
                assert nb.value > 2 * ((F + bf - 1) // bf if bf else 1), "no batch was rebuilt"
                lib.vmd_profile_ms(b"sasa_atoms", C.byref(nb))
                assert nb.value > ((F + bf - 1) // bf if bf else 1), "the walk of the repeated batch did not run again"
                same((rn.area(), rn.record()), one, bf)
    check(alone, restate(lib, coords, cell, lists, npoints=P), lists, "next to an rdf that repeats its batch", npoints=P, list_frames=[6])


def test_next_to_an_rdf_that_repeats_its_batch(emu_lib, oracle):
    overflow_case(emu_lib, oracle)


# ---- 6. the two-rank merge ------------------------------------------------------------------------------------------------------------------

def _merge_case():
    return HC.water_box(150, SC.CELLS[0][0], 6, seed=13), SC.water_lists(150)


def _merge_worker(rank, world, port, tmpdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import conftest
    from viamd_amd.dist import reduce_eval, shard_frames
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lib = V.VmdLib(conftest.EMU_LIB)
    coords, lists = _merge_case()
    F = coords.shape[0]
    ev = V.ScriptEval(F, sasa_ir(lib, lists))
    beg, end = shard_frames(F, rank, world)
    cell = V.make_unitcell(SC.CELLS[0][0])
    assert ev.frame_range(V.MolSystem(coords.shape[2], unitcell=cell), V.HostTrajectory(coords, cell), beg, end)
    own = ev.property_data(NAMES[1]).sasa_accumulators.copy()
    reduce_eval(ev)
    mean, frames = ev.sasa(NAMES[1])
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), own=own, merged=ev.property_data(NAMES[1]).sasa_accumulators.copy(),
             area=TG.rows(ev, NAMES[0])[:, 0], mean=mean, frames=frames)
    dist.destroy_process_group()


def test_two_rank_merge(emu_lib, tmp_path):
    """two evals over the halves of the frames, merged through the host collective: every rank's merged record and areas are the one-rank
    ones bit for bit"""
    import torch.multiprocessing as mp
    port = 51700 + (os.getpid() % 2000)
    mp.spawn(_merge_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    coords, lists = _merge_case()
    rn = run(emu_lib, lists, coords, SC.CELLS[0])
    check(rn, restate(emu_lib, coords, SC.CELLS[0], lists), lists, "one rank", list_frames=[0])
    total = np.zeros_like(rn.record())
    for r in range(2):
        z = np.load(tmp_path / f"rank{r}.npz")
        total = total + z["own"]
        assert np.array_equal(z["merged"], rn.record()) and int(z["frames"]) == coords.shape[0]
        assert np.array_equal(z["area"].view(np.int32), rn.area().view(np.int32))
        assert np.array_equal(z["mean"], rn.ev.sasa(NAMES[1])[0])
    assert np.array_equal(total, rn.record())


# ---- 7. the radii helper ----------------------------------------------------------------------------------------------------------------------

class _Topo:
    def __init__(self, elements):
        self.elements = np.array(elements)
        self.num_atoms = len(elements)


def test_vdw_radii_from_topology(host_lib):
    water = _Topo(["O", "H", "H"] * 3)
    for got in (script.vdw_radii_from_topology(water), script.vdw_radii_from_topology_native(water, lib=host_lib)):
        assert got.dtype == np.float32 and np.array_equal(got, SC.water_radii(3))
    pep = _Topo(["N", "h", "C", "H", "c", "O", "n", "S", "F", "P", "Cl", "CL", "br", "I", "Zn", "", "o"])
    want = np.array([1.55, 1.20, 1.70, 1.20, 1.70, 1.52, 1.55, 1.80, 1.47, 1.80, 1.75, 1.75, 1.85, 1.98, 2.00, 2.00, 1.52], np.float32)
    for got in (script.vdw_radii_from_topology(pep), script.vdw_radii_from_topology_native(pep, lib=host_lib)):
        assert np.array_equal(got, want)
    assert host_lib.vmd_topology_vdw_radii(None, None, 0) == 0 and "NULL" in host_lib.last_error()
    el = (C.c_char_p * 3)(b"O", b"H", b"H")
    assert host_lib.vmd_topology_vdw_radii(C.byref(L.TopologyC(3, el, None, None, None, None)), None, 0) == 3      # count only


# ---- 8. the IR: every refusal, the fingerprint field by field, the statement next to the others ---------------------------------------------

def test_ir_validation_errors(host_lib):
    lib = host_lib
    for sym in ("vmd_ir_add_sasa", "vmd_sasa_points", "vmd_eval_sasa", "vmd_eval_sasa_atoms", "vmd_topology_vdw_radii", "vmd_hip_sasa_atoms",
                "vmd_hip_sasa_brute", "vmd_hip_sasa_list", "vmd_hip_sasa_finish"):
        assert hasattr(lib, sym), sym
    ir = V.ScriptIR(lib)
    ok = dict(measured=[0, 3], measured_radius=[1.5, 1.2], env=[0, 1, 3], env_radius=[1.5, 1.2, 1.2], probe=1.4, npoints=96)

    def bad(match, names=NAMES, **kw):
        with pytest.raises(V.VmdError, match=match):
            ir.add_sasa_lists(names, **dict(ok, **kw))
    bad("measured list is empty", measured=[], measured_radius=[])
    bad("environment list is empty", env=[], env_radius=[])
    bad("negative", measured=[0, -1])
    bad("negative", env=[0, 1, -3])
    for r in (0.0, -1.0, float("inf"), float("nan")):
        bad("measured radius 1 must be finite and positive", measured_radius=[1.5, r])
        bad("environment radius 0 must be finite and positive", env_radius=[r, 1.2, 1.2])
    for pr in (-0.5, float("inf"), float("nan")):
        bad("probe radius must be finite and not negative", probe=pr)
    bad("plus the probe exceeds 8", measured_radius=[1.5, 6.7])
    bad("plus the probe exceeds 8", env_radius=[1.5, 1.2, 7.0], probe=1.5)
    for P in (0, 257, 100000):
        bad(r"\[1, 256\]", npoints=P)
    bad("name is empty", names=("", "pts"))
    bad("already defined", names=("x", "x"))
    names = (C.c_char_p * 2)(b"a", b"b")
    m, e_ = (np.array(v, np.int32) for v in ([0], [0, 1]))
    mr, er = (np.array(v, np.float32) for v in ([1.5], [1.5, 1.2]))
    ip = lambda x: x.ctypes.data_as(L.c_int32_p)
    fp_ = lambda x: x.ctypes.data_as(L.c_float_p)
    sites = L.SasaSitesC(1, ip(m), fp_(mr), 2, ip(e_), fp_(er))
    assert not lib.vmd_ir_add_sasa(None, names, C.byref(sites), 1.4, 96) and "ir is NULL" in lib.last_error()
    assert not lib.vmd_ir_add_sasa(ir.h, None, C.byref(sites), 1.4, 96) and "two property names" in lib.last_error()
    assert not lib.vmd_ir_add_sasa(ir.h, names, None, 1.4, 96) and "the sites" in lib.last_error()
    for s in (L.SasaSitesC(1, None, fp_(mr), 2, ip(e_), fp_(er)), L.SasaSitesC(1, ip(m), None, 2, ip(e_), fp_(er)),
              L.SasaSitesC(1, ip(m), fp_(mr), 2, None, fp_(er)), L.SasaSitesC(1, ip(m), fp_(mr), 2, ip(e_), None)):
        assert not lib.vmd_ir_add_sasa(ir.h, names, C.byref(s), 1.4, 96) and "empty" in lib.last_error()
    assert ir.property_count() == 0                                                # a refused statement leaves nothing behind
    ir.add_rmsd("g", [0, 1])
    bad("already defined", names=("g", "pts"))
    bad("already defined", names=("area", "g"))
    ir.add_sasa_lists(NAMES, **ok)
    ir.add_sasa_lists(("a0", "p0"), **dict(ok, probe=0.0, npoints=1))              # the ends of both ranges
    ir.add_sasa_lists(("a8", "p8"), **dict(ok, measured_radius=[1.5, 6.6], npoints=256))       # R = 8 exactly
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_rmsd("pts", [0, 1])
    assert ir.property_names()[:3] == ["g", "area", "pts"]
    assert ir.property_flags("area") == L.FLAG_TEMPORAL and ir.property_flags("pts") == L.FLAG_MAP
    with pytest.raises(ValueError):
        V.ScriptIR(lib).add_sasa(NAMES, [0, 1], [1.5])
    ir2 = V.ScriptIR(lib)
    ir2.add_sasa(NAMES, [0, 99], [1.5, 1.5])
    # (what follows evaluates: the emulator build always gets here, the product library only where there is a device - on a machine
    # without one its parameter ends above, as in tests/test_hbond.py)
    if lib.vmd_device_count() > 0:
        cell = ((10.0, 10.0, 10.0), (0.0, 0.0, 0.0), 7)
        with pytest.raises(V.VmdError, match="references atom 99"):
            Run(lib, ir2, np.zeros((1, 3, 10), np.float32), cell)
        rn = Run(lib, ir, np.zeros((2, 3, 10), np.float32), cell)
        ev = rn.ev
        with pytest.raises(V.VmdError, match="not a record of accessible surface points"):
            ev.sasa("area")
        with pytest.raises(V.VmdError, match="not a sasa property"):
            ev.sasa_atoms("g", rn.sysm, rn.traj, 0)
        with pytest.raises(V.VmdError, match="outside the trajectory"):
            ev.sasa_atoms("area", rn.sysm, rn.traj, 2)
        assert not lib.vmd_eval_sasa(ev.h, b"nope", None, None) and "unknown property" in lib.last_error()
        assert not lib.vmd_eval_sasa(None, b"pts", None, None) and "NULL" in lib.last_error()
        assert lib.vmd_eval_sasa(ev.h, b"pts", None, None)                         # every output may be left out
        failed = C.c_size_t(-1).value
        assert lib.vmd_eval_sasa_atoms(ev.h, b"nope", None, rn.traj.interface(), 0, None, 0) == failed
        assert lib.vmd_eval_sasa_atoms(None, b"pts", None, rn.traj.interface(), 0, None, 0) == failed
        assert lib.vmd_eval_sasa_atoms(ev.h, b"pts", None, rn.traj.interface(), 0, None, 0) == 2        # either name of the statement
        # all atoms at the origin: the environment's three entries coincide and answer as entry 0 (atom 0, R 2.9).  Measured atom 0 is
        # itself; measured atom 3 (R 2.6) lies at the centre of the larger atom 0
        assert list(ev.sasa_atoms("pts", rn.sysm, rn.traj, 1)) == [96, 0]
        pd = ev.property_data("pts")
        assert pd.dim == (3, 1, 0, 0) and pd.unit_str == ("", "") and list(pd.sasa_accumulators) == [192, 0, 2]
        assert ev.property_data("area").dim == (2, 1, 0, 0) and ev.property_data("area").unit_str == ("", "Å²")
        mean, F = ev.sasa("pts")
        assert F == 2 and mean[1] == 0.0 and abs(mean[0] - 4.0 * math.pi * float(np.float32(1.5) + np.float32(1.4)) ** 2) < 1e-9
        with pytest.raises(V.VmdError, match="accessible surface points"):
            ev.export_table("/dev/null", "pts", "csv")


def test_fingerprint_work_and_atoms(host_lib):
    assert TR._old_ir(host_lib).fingerprint() == TR.PARENT_FINGERPRINT              # an IR without the forms keeps its fingerprint

    def fp(**kw):
        ir = V.ScriptIR(host_lib)
        a = dict(names=NAMES, measured=[0, 3], measured_radius=[1.5, 1.2], env=[0, 1, 3], env_radius=[1.5, 1.2, 1.2], probe=1.4, npoints=96)
        a.update(kw)
        ir.add_sasa_lists(**a)
        return ir.fingerprint(), int(host_lib.vmd_ir_work_per_frame(ir.h))
    f0, w0 = fp()
    variants = dict(name0=fp(names=("x", "pts")), name1=fp(names=("area", "x")), measured=fp(measured=[0, 4]), env=fp(env=[0, 2, 3]),
                    order=fp(env=[1, 0, 3]), fewer=fp(env=[0, 3], env_radius=[1.5, 1.2]), probe=fp(probe=1.5), npoints=fp(npoints=97),
                    rmeas0=fp(measured_radius=[1.55, 1.2]), rmeas1=fp(measured_radius=[1.5, 1.25]), renv0=fp(env_radius=[1.55, 1.2, 1.2]),
                    renv1=fp(env_radius=[1.5, 1.25, 1.2]), renv2=fp(env_radius=[1.5, 1.2, 1.25]),
                    # radius and probe are hashed apart: the same R from another split is another statement
                    split=fp(measured_radius=[1.4, 1.1], env_radius=[1.4, 1.1, 1.1], probe=1.5))
    assert len({f0} | {v[0] for v in variants.values()}) == 1 + len(variants), variants
    assert w0 == 2 * (1 + 3) + 2 * 3 and variants["fewer"][1] == 2 * (1 + 3) + 2 * 2 and variants["npoints"][1] == 2 * (1 + 4) + 2 * 3
    # hbonds over the same lists is another statement (codes 16 / 17 against 14 / 15)
    ir = V.ScriptIR(host_lib)
    ir.add_hbonds(NAMES, [0, 3], [1, 4], [0, 1, 3], 3.5, 150.0)
    assert ir.fingerprint() != f0
    ir = TR._old_ir(host_lib)
    w_old = int(host_lib.vmd_ir_work_per_frame(ir.h))
    ir.add_sasa_lists(NAMES, [0, 3], [1.5, 1.2], [0, 1, 3], [1.5, 1.2, 1.2])
    assert ir.fingerprint() != TR.PARENT_FINGERPRINT and int(host_lib.vmd_ir_work_per_frame(ir.h)) == w_old + w0
    assert list(ir.geometry_atoms("area")) == [0, 3, 0, 1, 3]                      # measured, then environment
    assert list(ir.geometry_atoms("area", 0)) == [0, 3, 0, 1, 3] and ir.geometry_atoms("area", 1).size == 0
    assert ir.geometry_atoms("pts").size == 0
    # add_sasa: the measured set as positions into the environment
    a, b = V.ScriptIR(host_lib), V.ScriptIR(host_lib)
    a.add_sasa(NAMES, [5, 6, 7], [1.5, 1.2, 1.2], measured=[0, 2])
    b.add_sasa_lists(NAMES, [5, 7], [1.5, 1.2], [5, 6, 7], [1.5, 1.2, 1.2])
    assert a.fingerprint() == b.fingerprint() and list(a.geometry_atoms("area")) == [5, 7, 5, 6, 7]


def next_to_the_other_forms(lib, oracle, device=False):
    """VIAMD's default script plus rmsd, ramachandran, secondary_structure, rmsf and hbonds statements, with and without a sasa statement
    in the same IR: every other property is bit-identical, the new ones equal the restatement and an IR of their own"""
    atoms, blob, box, F = 6001, 200, 30.0, 4
    coords, topo = TG.blob_system(oracle, n_atoms=atoms, n_blob=blob, box=box, F=F, seed=5)
    names = np.array(["N", "CA", "C", "O", "CB", "H", "HA", "HB1", "CG", "HG"])
    topo.names = np.where(np.arange(atoms) < blob, names[np.arange(atoms) % 10], topo.elements)
    bb = script.backbone_from_topology(topo)
    o = script.backbone_oxygens_from_topology(topo, bb)
    el = np.array([str(e).upper() for e in topo.elements])
    wo = np.nonzero((el == "O") & (np.arange(atoms) >= blob))[0]
    bonds = [(int(i), int(i) + k) for i in wo for k in (1, 2) if i + k < atoms and el[i + k] == "H"]
    sites = script.hbond_sites_from_topology(topo, bonds)
    rad = script.vdw_radii_from_topology(topo)
    lists = lists_of(np.arange(atoms, dtype=np.int32), rad, measured=np.arange(blob))        # the blob's area in its solvent
    evs = []
    for with_sasa in (False, True):
        ir = script.compile_script_native(TG.VIAMD_DEFAULT_SCRIPT + TR.RM_LINE, topo, lib=lib, **OPT_INS)
        ir.add_ramachandran(("bb", "rama"), **bb)
        ir.add_secondary_structure(("ss", "sspop"), bb["n"], bb["ca"], bb["c"], o, bb["range_offsets"], bb["rama_class"])
        ir.add_rmsf("fl", np.arange(blob, dtype=np.int32))
        ir.add_hbonds(("nhb", "occ"), sites["donor"], sites["hydrogen"], sites["acceptor"], HC.R_DA, HC.ANGLE)
        if with_sasa:
            ir.add_sasa(NAMES, lists["env"], lists["env_radius"], measured=np.arange(blob))
        evs.append(TG.evaluate(lib, ir, coords, box, topo.mass, device=device))
    plain, both = evs
    props = plain.ir.property_names()
    assert props == ["d1", "a1", "r", "v", "lin", "plan", "iso", "rm", "bb", "rama", "ss", "sspop", "fl", "nhb", "occ"]
    assert both.ir.property_names() == props + list(NAMES)
    for name in props:
        a, b = plain.property_data(name), both.property_data(name)
        assert a.dim == b.dim and a.fingerprint == b.fingerprint, name
        assert np.array_equal(a.values.view(np.int32), b.values.view(np.int32)), name
        if a.c.counts:
            assert np.array_equal(a.counts, b.counts), name
    cell = ((box, box, box), (0.0, 0.0, 0.0), 7)
    want = restate(lib, coords, cell, lists)
    print(f"blob system: {int(want['record'][:-1].sum())} accessible points, near the thresholds {want['near_s']} / {want['near_t']}")
    assert np.array_equal(TG.rows(both, NAMES[0])[:, 0].view(np.int32), want["area"].view(np.int32))
    assert np.array_equal(both.property_data(NAMES[1]).sasa_accumulators, want["record"])
    alone = run(lib, lists, coords, cell, device)
    same((alone.area(), alone.record()), (TG.rows(both, NAMES[0])[:, 0], both.property_data(NAMES[1]).sasa_accumulators), "an IR of its own")


def test_next_to_the_other_forms_on_the_emulator(emu_lib, oracle):
    next_to_the_other_forms(emu_lib, oracle)

