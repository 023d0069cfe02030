"""Hydrogen bonds on the emulator build and in the host-only entry points.  The rule is EXACT EQUALITY with the numpy
restatement (tests/hbond_ref.py) for all three outputs - the counts per frame, every accumulator of the occupancy record, the pair lists -
and every launch choice (walk or all pairs, batch size, call pattern) bit-identical to the others.  Every check prints how many candidate
pairs lie within 4 ulp of the distance threshold and how many distance hits within 4 ulp of the angle's, so that a reader sees the equality
was exercised.  Scenarios: a hand-placed water dimer across the faces, an edge and a corner of a cell, tilted and with open axes; the size
edges of both lists in a roomy cell, in one just large enough for a grid and in one too small; planted thresholds under both
spec_within_closed settings and at 90 / 180 degrees; identity (self pairs, an acceptor that is a hydrogen, coincident acceptors, a hydrogen
in another image, k_sorted_atoms on face atoms); the call patterns; a batch repeated for a bucket overflow; the two-rank merge; the
topology helper; and the IR cases - every refusal, the fingerprint field by field, the statement next to the default script and the other
forms.  tests/test_hbond_gpu.py runs the same scenario functions on the device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import viamd_amd as V
from viamd_amd import _lib as L
from viamd_amd import script

import cases
import cell_build_cases as CB
import hbond_cases as HC
import hbond_ref as R
import test_geometry as TG
import test_rmsd as TR
from test_rama import OPT_INS, Option

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nhb", "occ")
WALK, BRUTE = dict(shell_brute_below=0), dict(shell_brute_below=1 << 30)
NEAR = {}                        # what -> (candidates near the distance threshold, hits near the angle threshold), as printed


class Options:
    def __init__(self, lib, **kw):
        self.opts = [Option(lib, k, v) for k, v in kw.items()]

    def __enter__(self):
        for o in self.opts:
            o.__enter__()

    def __exit__(self, *exc):
        for o in reversed(self.opts):
            o.__exit__(*exc)


def hb_ir(lib, sites, r=HC.R_DA, angle=HC.ANGLE, names=NAMES):
    ir = V.ScriptIR(lib)
    ir.add_hbonds(names, sites["donor"], sites["hydrogen"], sites["acceptor"], r, angle)
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

    def counts(self, name=NAMES[0]):
        return TG.rows(self.ev, name)[:, 0]

    def record(self, name=NAMES[1]):
        return self.ev.property_data(name).hbond_accumulators.copy()

    def pairs(self, frame, name=NAMES[0]):
        return self.ev.hbond_pairs(name, self.sysm, self.traj, frame)


def run(lib, sites, coords, cell, device=False, r=HC.R_DA, angle=HC.ANGLE, **kw):
    return Run(lib, hb_ir(lib, sites, r, angle), coords, cell, device, **kw)


def ref_box(cell):
    box, tilt, flags = cell
    return (tuple(box) + tuple(tilt) if any(tilt) else box), flags


def restate(coords, cell, sites, r=HC.R_DA, angle=HC.ANGLE, closed=False, frames=None):
    bx, flags = ref_box(cell)
    return R.evaluate(coords, bx, sites["donor"], sites["hydrogen"], sites["acceptor"], r, angle, closed=closed, flags=flags, frames=frames)


def check(rn, want, sites, what, list_frames=None):
    """the three outputs against the restatement `want`, exactly, and the invariants of every scenario"""
    npairs, nacc = len(sites["donor"]), len(sites["acceptor"])
    got_c, got_r = rn.counts(), rn.record()
    NEAR[what] = (want["near_d"], want["near_a"])
    print(f"{what}: {int(want['counts'].sum())} bonds in {int(want['record'][-1])} frames, {want['near_d']} candidate pairs within 4 ulp of "
          f"r_da, {want['near_a']} distance hits within 4 ulp of the angle threshold")
    assert got_c.dtype == np.float32 and np.array_equal(got_c.view(np.int32), want["counts"].view(np.int32)), what
    assert got_r.shape == (npairs + nacc + 1,) and np.array_equal(got_r, want["record"]), what
    # invariants: donor rows, acceptor rows and the counts of the evaluated frames add up to the same number; the frames row
    frames = sorted(want["pairs"])
    assert int(got_r[:npairs].sum()) == int(got_r[npairs:-1].sum()), what
    if int(got_r[-1]) == len(frames):          # (no frame twice: the temporal rows then say what the record says)
        assert int(got_r[:npairs].sum()) == int(got_c[frames].sum()), what
    don, acc, F = rn.ev.hbonds(NAMES[1])
    assert F == int(got_r[-1]) and np.array_equal(don, got_r[:npairs] / max(F, 1)) and np.array_equal(acc, got_r[npairs:-1] / max(F, 1)), what
    for f in (frames if list_frames is None else list_frames):
        got = rn.pairs(f)
        assert got.shape == want["pairs"][f].shape and np.array_equal(got, want["pairs"][f]), (what, f)
        assert len(got) == int(want["counts"][f]), (what, f)
    return got_c, got_r


def same(a, b, what):
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1]), what


# ---- 1. a known answer ------------------------------------------------------------------------------------------------------------------------

def known_answer(lib, device=False):
    """The dimer of hbond_cases has one bond, O0-H1 ... O3.  Frame by frame it is moved so that the bond crosses each face, an edge and a
    corner of a cubic cell; then the same in a tilted cell and in one with open axes (where a bond across the open face is none)."""
    rng = np.random.default_rng(2)
    L_ = 20.0
    spots = [(10.0, 10.0, 10.0), (L_ - 1.5, 10.0, 10.0), (10.0, L_ - 1.5, 10.0), (10.0, 10.0, L_ - 1.5), (L_ - 1.5, L_ - 1.0, 10.0),
             (L_ - 1.0, L_ - 1.0, L_ - 1.0), (-1.5, 3.0 * L_ + 0.5, -L_ - 1.0)]
    axes = [np.eye(3), np.eye(3)[[1, 0, 2]], np.eye(3)[[2, 1, 0]]]                      # the bond along x, y, z
    frames = []
    for k, sp in enumerate(spots):
        rot = axes[k % 3] if k < 4 else HC.rotation(rng)
        frames.append(HC.dimer(sp, rot).T)
    coords = np.stack(frames).astype(np.float32)
    for cell in (((L_, L_, L_), (0.0, 0.0, 0.0), 7), ((L_, L_, L_), (4.0, -2.0, 3.0), 7)):
        want = restate(coords, cell, HC.DIMER_SITES)
        assert list(want["counts"]) == [1.0] * len(spots)
        for f in range(len(spots)):
            assert [tuple(t) for t in want["pairs"][f]] == [HC.DIMER_BOND]
        one = None
        for route in (dict(), WALK, BRUTE):
            with Options(lib, **route):
                got = check(run(lib, HC.DIMER_SITES, coords, cell, device), want, HC.DIMER_SITES, f"dimer, tilt {cell[1]}, {route}")
            one = one or got
            same(got, one, route)
        assert list(one[1]) == [len(spots), 0, 0, 0, 0, len(spots), len(spots)]          # pair 0 donates, acceptor 1 (O3) accepts
    # open axes: x open.  The frames whose bond crosses the x face lose it (no image across an open face), the others keep it
    cell = ((L_, L_, L_), (0.0, 0.0, 0.0), 6)
    want = restate(coords, cell, HC.DIMER_SITES)
    assert want["counts"][0] == 1 and want["counts"][2] == 1 and want["counts"][3] == 1
    for route in (dict(), WALK, BRUTE):
        with Options(lib, **route):
            check(run(lib, HC.DIMER_SITES, coords, cell, device), want, HC.DIMER_SITES, f"dimer, x open, {route}")


def test_known_answer_on_the_emulator(emu_lib):
    known_answer(emu_lib)


# ---- 2. size edges ----------------------------------------------------------------------------------------------------------------------------

N_W = 500
SWEEP = [(n, k) for n in HC.NPAIRS for k in (65, 481)] + [(257, k) for k in HC.NACC if k not in (65, 481)] + [(1, 1), (64, 479), (65, 480)]


def size_sweep(lib, ci, device=False):
    """npairs x nacc of hbond_cases in cell ci: the default route (all pairs below 480 acceptors, the walk from there), then the walk and all
    pairs forced through shell_brute_below - one answer; batch_frames 1 and 2 on a few"""
    cell = HC.CELLS[ci]
    coords = HC.water_box(N_W, cell[0], 3, seed=3 + ci)
    for npairs, nacc in SWEEP:
        sites = HC.subset_sites(N_W, npairs, nacc, seed=100 * ci + npairs + nacc)
        want = restate(coords, cell, sites)
        what = f"cell {ci}, {npairs} pairs x {nacc} acceptors"
        one = check(run(lib, sites, coords, cell, device), want, sites, what, list_frames=[1])
        for route in (WALK, BRUTE):
            with Options(lib, **route):
                rn = run(lib, sites, coords, cell, device)
                same((rn.counts(), rn.record()), one, (what, route))
        if npairs in (1, 257):
            for bf in (1, 2):
                with Options(lib, batch_frames=bf, **WALK):
                    rn = run(lib, sites, coords, cell, device)
                    same((rn.counts(), rn.record()), one, (what, bf))
        if device and npairs == 257:
            rn = run(lib, sites, coords, cell)
            same((rn.counts(), rn.record()), one, (what, "host-staged"))


@pytest.mark.parametrize("ci", range(len(HC.CELLS)))
def test_size_edges_on_the_emulator(emu_lib, ci):
    size_sweep(emu_lib, ci)


def tight_boxes(lib, device=False):
    """A cell just large enough for a grid at r_da (two pencils per axis: every neighbour pencil is met under two images) and one too
    small, where the walk cannot be had and all pairs answer whatever is asked: dense, most pairs are distance hits"""
    for edge, grid in ((HC.TIGHT, True), (HC.TOO_SMALL, False)):
        cell = ((edge, edge, edge), (0.0, 0.0, 0.0), 7)
        n_w = 90
        coords = HC.water_box(n_w, cell[0], 3, seed=11)
        sites = HC.water_sites(n_w)
        want = restate(coords, cell, sites)
        one = None
        for route in (dict(), WALK, BRUTE):
            lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
            try:
                with Options(lib, **route):
                    got = check(run(lib, sites, coords, cell, device), want, sites, f"edge {edge}, {route}", list_frames=[0])
            finally:
                lib.vmd_profile_enable(False)
            n = C.c_uint64(0)
            lib.vmd_profile_ms(b"hbond_atoms", C.byref(n))
            assert (n.value > 0) == (grid and route is WALK), (edge, route, n.value)
            one = one or got
            same(got, one, (edge, route))


def test_tight_boxes_on_the_emulator(emu_lib):
    tight_boxes(emu_lib)


# ---- 3. thresholds ----------------------------------------------------------------------------------------------------------------------------

def steps(v, lo, hi):
    out, x = [], np.float32(v)
    for _ in range(-lo):
        x = np.nextafter(x, np.float32(-np.inf))
    for _ in range(hi - lo + 1):
        out.append(x)
        x = np.nextafter(x, np.float32(np.inf))
    return out


def planted_thresholds(angle):
    """One donor, its hydrogen and one acceptor per FRAME, all at coordinates of a few Angstrom so that one ulp is a fine step.  First
    group: the acceptor on the hydrogen's axis at r_da moved by -4 .. 4 ulp, from two donor positions (the angle is 180 degrees: only
    the distance decides).  Second group: the acceptor at 3 A on the axis, the hydrogen 1 A from D turned off the axis to where the
    D-H...A angle is `angle` (found in float64 for the fp32 x it really has), its y moved by -12 .. 12 ulp (only the angle decides)."""
    r = np.float32(HC.R_DA)
    frames = []
    for dx in steps(r, -4, 4):
        for base in (5.0, 4.0 + 1.0 / 3.0):
            frames.append([(base, 2.0, 5.0), (base + 1.0, 2.0, 5.0), (float(np.float32(base) + dx), 2.0, 5.0)])

    def angle_at(hx, hy):
        h = np.array([hx, hy])
        u, v = -h, np.array([3.0, 0.0]) - h
        return np.degrees(np.arccos(np.clip(u @ v / np.linalg.norm(u) / np.linalg.norm(v), -1, 1)))
    lo, hi = 0.0, np.pi / 2
    for _ in range(80):
        t = 0.5 * (lo + hi)
        lo, hi = (t, hi) if angle_at(np.cos(t), np.sin(t)) > angle else (lo, t)
    x32 = np.float32(1.0 + np.cos(lo))
    hx = float(x32) - 1.0
    lo, hi = 0.0, 1.5
    for _ in range(80):
        t = 0.5 * (lo + hi)
        lo, hi = (t, hi) if angle_at(hx, t) > angle else (lo, t)
    for y32 in steps(np.float32(1.0 + lo), -12, 12):
        frames.append([(1.0, 1.0, 5.0), (float(x32), float(y32), 5.0), (4.0, 1.0, 5.0)])
    coords = np.asarray(frames, np.float64).transpose(0, 2, 1).astype(np.float32)
    return coords, dict(donor=np.array([0], np.int32), hydrogen=np.array([1], np.int32), acceptor=np.array([2], np.int32))


def thresholds(lib, device=False):
    for angle in (90.0, 120.0, 150.0, 180.0):
        coords, sites = planted_thresholds(angle)
        cell = ((16.0, 16.0, 16.0), (0.0, 0.0, 0.0), 7)
        for closed in (0, 1):
            want = restate(coords, cell, sites, angle=angle, closed=bool(closed))
            assert want["near_d"] >= 9 and (angle == 90.0 or want["near_a"] >= 1), (angle, want["near_d"], want["near_a"])
            assert 0 < want["counts"][:18].sum() < 18 and (angle in (90.0, 180.0) or 0 < want["counts"][18:].sum() < 25), (angle, want["counts"])
            # (at 180 degrees a few ulp off the axis change cos^2 by 1e-12: the rounding of the products decides, the same way on both sides)
            one = None
            for route in (WALK, BRUTE):
                with Options(lib, spec_within_closed=closed, **route):
                    got = check(run(lib, sites, coords, cell, device, angle=angle), want, sites, f"thresholds, {angle} degrees, closed {closed}, "
                                f"{route}")
                one = one or got
                same(got, one, (angle, closed, route))
    assert any(NEAR[k][1] > 0 for k in NEAR if k.startswith("thresholds"))


def test_thresholds_on_the_emulator(emu_lib):
    thresholds(emu_lib)


# ---- 4. identity ------------------------------------------------------------------------------------------------------------------------------

def identity(lib, device=False):
    """A water box where every O donates and accepts (the self pair is never a bond); hydrogens in the acceptor list (an acceptor that is
    some pair's hydrogen); two atoms made coincident bit for bit and an atom listed twice (D-HB-COINCIDENT: the lowest entry answers);
    hydrogens whose raw position is in another image than their donor's (hbond_cases.water_box spills over the faces, and a few hydrogens
    are moved by a whole cell here)."""
    cell = HC.CELLS[0]
    n_w = 400
    coords = HC.water_box(n_w, cell[0], 3, seed=5).copy()
    sites = HC.water_sites(n_w)
    Lx = np.float32(cell[0][0])
    coords[:, 0, 1:300:3] += Lx                                           # the first hydrogen of a hundred waters: one cell further
    coords[:, 2, 2:300:6] -= np.float32(2.0) * np.float32(cell[0][2])
    want = restate(coords, cell, sites)
    assert want["counts"].sum() > 100
    moved = restate(HC.water_box(n_w, cell[0], 3, seed=5), cell, sites)
    assert np.array_equal(want["counts"], moved["counts"])               # whole cells move nothing
    for t in want["pairs"].values():
        assert (t[:, 0] != t[:, 2]).all()
    one = None
    for route in (WALK, BRUTE):
        with Options(lib, **route):
            got = check(run(lib, sites, coords, cell, device), want, sites, f"water box, every O both, {route}", list_frames=[0, 2])
        one = one or got
        same(got, one, route)
    # hydrogens accept too; the oxygen that accepts most (a) gets another oxygen (b) put on it bit for bit, b listed in front; atom 6 is
    # listed twice.  Entry 1 (b) answers for a and for b's own later entry, entry 0 for both 6s
    rec = want["record"][len(sites["donor"]):-1]
    a = int(sites["acceptor"][int(np.argmax(rec))])
    b = (a + 3 * 150) % (3 * n_w)
    c2 = coords.copy()
    c2[:, :, b] = c2[:, :, a]
    acc = np.concatenate([[6, b], sites["acceptor"], np.arange(1, 200, 3)]).astype(np.int32)
    s2 = dict(sites, acceptor=acc)
    want = restate(c2, cell, s2)
    rec = want["record"][len(s2["donor"]):-1]
    assert rec[1] >= 2 and rec[2 + a // 3] == 0 and rec[2 + b // 3] == 0 and rec[2 + 2] == 0
    one = None
    for route in (WALK, BRUTE):
        with Options(lib, **route):
            got = check(run(lib, s2, c2, cell, device), want, s2, f"coincident acceptors, {route}", list_frames=[1])
        one = one or got
        same(got, one, route)


def test_identity_on_the_emulator(emu_lib):
    identity(emu_lib)


def sorted_atoms_identity(lib, O, gpu=False):
    """k_sorted_atoms on the face systems of the cell-build cases (atoms on cell faces, at -0.0, at nextafter(L, 0), a million cells away),
    periodic and with an open axis, plus two entries made coincident: no slot is left unclaimed, every slot names an entry whose wrapped
    coordinates are the slot's bit for bit, and it is the lowest such entry"""
    for seed, flags, grid in ((1, 7, CB.grid3(7, 5, 4)), (2, 5, CB.grid3(9, 3, 6)), (3, 7, CB.grid3(1, 2, 2))):
        N, B = 700, 3
        sel = CB.sel_list(seed, 300, N)
        sy = CB.System(seed, N, B, grid, sel, flags=flags)
        sy.coords[:, :, sel.atoms[17]] = sy.coords[:, :, sel.atoms[250]]
        sy.coords[:, :, sel.atoms[100]] = sy.coords[:, :, sel.atoms[250]]
        _, _, nsel, npad, host = CB._common(sy)
        words = int(lib.vmd_hip_cells_scratch_words(grid, nsel))
        buf = CB.Buffers(gpu, cc=np.zeros(B * (grid.ncell + 1), np.uint32), rank=np.zeros(B * max(words, 1), np.uint32),
                         ident=np.zeros(B * npad, np.uint32), **host)
        assert lib.vmd_hip_cells_build(None, buf["xyz"], 3 * N, N, buf["g9"], flags, B, buf["sel"], nsel, npad, grid, buf["cc"], buf["rank"],
                                       buf["cs"], buf["srt"], None) == 0
        assert lib.vmd_hip_sorted_atoms(None, buf["xyz"], 3 * N, N, buf["g9"], flags, B, buf["sel"], nsel, buf["srt"], buf["cs"], npad, grid,
                                        buf["ident"], None) == 0
        ident = buf.fetch("ident").reshape(B, npad)
        srt = buf.fetch("srt")[:B * 3 * npad].reshape(B, 3, npad).view(np.int32)
        ref = sy.reference(O)[0].view(np.int32)                            # [B][3][nsel] wrapped, by list entry
        for b in range(B):
            claimed = ident[b, :nsel]
            assert (claimed != 0xffffffff).all() and (claimed < nsel).all(), (seed, b)
            assert (ident[b, nsel:] == 0xffffffff).all()
            assert np.array_equal(ref[b][:, claimed], srt[b][:, :nsel]), (seed, b)
            first = {}
            for t, key in enumerate(map(tuple, ref[b].T)):
                first.setdefault(key, t)
            assert [first[tuple(k)] for k in srt[b][:, :nsel].T] == list(claimed), (seed, b)
            assert sorted(set(claimed)) == sorted(set(first.values()))
            assert 100 not in claimed and 250 not in claimed and (claimed == 17).sum() == 3


def test_sorted_atoms_leaves_no_slot_unclaimed(emu_lib, oracle):
    sorted_atoms_identity(emu_lib, oracle)


# ---- 5. call patterns -------------------------------------------------------------------------------------------------------------------------

def call_patterns(lib, device=False):
    """one call; many small ranges in shuffled order; pool threads; clear_data then again; a frame evaluated twice counts twice; a frame
    mask (frames never evaluated read +0 and are not counted); a source's frame blocks"""
    cell = HC.CELLS[0]
    n_w, F = 300, 8
    coords = HC.water_box(n_w, cell[0], F, seed=9)
    sites = HC.water_sites(n_w)
    want = restate(coords, cell, sites)
    with Options(lib, **WALK):
        first = run(lib, sites, coords, cell, device)
        one = check(first, want, sites, "one call", list_frames=[0, F - 1])
        order = [(f, f + 1) for f in np.random.default_rng(4).permutation(F)]
        for kw in (dict(ranges=[(5, 8), (0, 2), (2, 5)]), dict(ranges=order), dict(pooled=(16, 1)), dict(pooled=(4, 2))):
            rn = run(lib, sites, coords, cell, device, **kw)
            same((rn.counts(), rn.record()), one, kw)
        with Options(lib, batch_frames=3):
            rn = run(lib, sites, coords, cell, device)
            same((rn.counts(), rn.record()), one, "batch_frames 3")
        # the single-frame query touches nothing accumulated
        before = first.record()
        first.pairs(3)
        assert np.array_equal(first.record(), before) and np.array_equal(first.counts().view(np.int32), one[0].view(np.int32))
        first.ev.clear_data()
        assert not first.record().any() and first.ev.hbonds(NAMES[1])[2] == 0 and not first.ev.hbonds(NAMES[1])[0].any()
        assert first.ev.frame_range(first.sysm, first.traj, 0, F)
        same((first.counts(), first.record()), one, "clear_data, then again")
        # frames 2 .. 4 alone: a partial record, the other rows +0; then the same frames again: counted twice
        part = run(lib, sites, coords, cell, device, ranges=[(2, 5)])
        wp = restate(coords, cell, sites, frames=[2, 3, 4])
        got = check(part, wp, sites, "frames 2 .. 4", list_frames=[2])
        assert not got[0][:2].any() and not got[0][5:].any() and got[1][-1] == 3
        assert part.ev.frame_range(part.sysm, part.traj, 2, 5)
        check(part, restate(coords, cell, sites, frames=[2, 3, 4, 2, 3, 4]), sites, "frames 2 .. 4 twice", list_frames=[])
        assert np.array_equal(part.record(), 2 * got[1])
        # a source evaluated in blocks of two frames lends frames 2 .. 3
        ir = hb_ir(lib, sites)
        src = V.ScriptEval(F, ir)
        src.set_block_frames(2)
        assert src.frame_range(first.sysm, first.traj, 0, F)
        assert np.array_equal(src.property_data(NAMES[1]).hbond_accumulators, one[1])
        flt = V.ScriptEval(F, ir)
        flt.set_block_frames(2)
        flt.set_source(src)
        assert flt.frame_range(first.sysm, first.traj, 2, 4) and flt.frame_stats()[1] > 0
        assert np.array_equal(flt.property_data(NAMES[1]).hbond_accumulators, restate(coords, cell, sites, frames=[2, 3])["record"])


def test_call_patterns_on_the_emulator(emu_lib):
    call_patterns(emu_lib)


def overflow_case(lib, O, device=False):
    """test_rmsf.overflow_case's construction: the middle frames pile every oxygen into one pencil, a bucket sized from the batch's ends
    overflows and the batch is repeated.  The occupancy is added with atomics behind the overflow flag: it must not count that batch
    twice - the record is that of an IR without the rdf, which no overflow ever touches (all pairs)."""
    n, box, F = 3000, 60.0, 12
    coords = cases.water_box(O, 5, n, box, F)
    o = cases.oxygen(n)
    rng = np.random.default_rng(3)
    for f in (5, 6, 7):
        coords[f][:, o] = rng.uniform(1.0, 11.0, (3, o.size)).astype(np.float32)
    sites = HC.water_sites(n // 3)
    sites = dict(donor=sites["donor"][:600], hydrogen=sites["hydrogen"][:600], acceptor=sites["acceptor"])
    cell = ((box, box, box), (0.0, 0.0, 0.0), 7)
    with Options(lib, **BRUTE):
        alone = run(lib, sites, coords, cell, device)
    one = (alone.counts(), alone.record())
    assert one[1][-1] == F and one[1][:-1].any()
    with Options(lib, cells_small=0, cells_cap_sample=2, **WALK):
        for bf in (0, 4):
            with Options(lib, batch_frames=bf):
                ir = hb_ir(lib, sites)
                ir.add_rdf("goo", o, o, (0.0, 12.0))
                lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
                try:
                    rn = Run(lib, ir, coords, cell, device)
                finally:
                    lib.vmd_profile_enable(False)
                nb = C.c_uint64(0)
                lib.vmd_profile_ms(b"cells_build", C.byref(nb))
                assert nb.value > 2 * ((F + bf - 1) // bf if bf else 1), "no batch was rebuilt"
                lib.vmd_profile_ms(b"hbond_atoms", C.byref(nb))
                assert nb.value > ((F + bf - 1) // bf if bf else 1), "the walk of the repeated batch did not run again"
                same((rn.counts(), rn.record()), one, bf)
    check(alone, restate(coords, cell, sites), sites, "next to an rdf that repeats its batch", list_frames=[6])


def test_next_to_an_rdf_that_repeats_its_batch(emu_lib, oracle):
    overflow_case(emu_lib, oracle)


# ---- 6. the two-rank merge ------------------------------------------------------------------------------------------------------------------

def _merge_case():
    return HC.water_box(200, HC.CELLS[0][0], 6, seed=13), HC.water_sites(200)


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
    coords, sites = _merge_case()
    F = coords.shape[0]
    ev = V.ScriptEval(F, hb_ir(lib, sites))
    beg, end = shard_frames(F, rank, world)
    cell = V.make_unitcell(HC.CELLS[0][0])
    assert ev.frame_range(V.MolSystem(coords.shape[2], unitcell=cell), V.HostTrajectory(coords, cell), beg, end)
    own = ev.property_data(NAMES[1]).hbond_accumulators.copy()
    reduce_eval(ev)
    don, acc, frames = ev.hbonds(NAMES[1])
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), own=own, merged=ev.property_data(NAMES[1]).hbond_accumulators.copy(),
             counts=TG.rows(ev, NAMES[0])[:, 0], don=don, frames=frames)
    dist.destroy_process_group()


def test_two_rank_merge(emu_lib, tmp_path):
    """two evals over the halves of the frames, merged through the host collective: every rank's merged record and counts are the
    one-rank ones bit for bit"""
    import torch.multiprocessing as mp
    port = 49600 + (os.getpid() % 2000)
    mp.spawn(_merge_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    coords, sites = _merge_case()
    rn = run(emu_lib, sites, coords, HC.CELLS[0])
    check(rn, restate(coords, HC.CELLS[0], sites), sites, "one rank", list_frames=[0])
    total = np.zeros_like(rn.record())
    for r in range(2):
        z = np.load(tmp_path / f"rank{r}.npz")
        total = total + z["own"]
        assert np.array_equal(z["merged"], rn.record()) and int(z["frames"]) == coords.shape[0]
        assert np.array_equal(z["counts"].view(np.int32), rn.counts().view(np.int32))
        assert np.array_equal(z["don"], rn.ev.hbonds(NAMES[1])[0])
    assert np.array_equal(total, rn.record())


# ---- 7. the topology helper -------------------------------------------------------------------------------------------------------------------

class _Topo:
    def __init__(self, elements):
        self.elements = np.array(elements)
        self.num_atoms = len(elements)


def test_sites_from_topology(host_lib):
    n_w = 4
    water = _Topo(["O", "H", "H"] * n_w)
    bonds = [(3 * w, 3 * w + k) for w in range(n_w) for k in (2, 1)] + [(1, 0)]       # unordered, one bond twice and reversed
    want = HC.water_sites(n_w)
    for got in (script.hbond_sites_from_topology(water, bonds), script.hbond_sites_from_topology_native(water, bonds, lib=host_lib)):
        for k in ("donor", "hydrogen", "acceptor"):
            assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    # a small peptide: N-H donates, the hydroxyl O-H donates, C-H does not; N, O and F accept, S and C do not
    #          0    1    2    3    4    5    6    7    8    9    10   11   12
    pep = _Topo(["N", "H", "C", "H", "C", "O", "N", "h", "C", "o", "H", "S", "F"])
    bonds = [(0, 1), (0, 2), (2, 3), (2, 4), (4, 5), (4, 6), (7, 6), (6, 8), (8, 9), (9, 10), (8, 11), (11, 12)]
    for got in (script.hbond_sites_from_topology(pep, bonds), script.hbond_sites_from_topology_native(pep, bonds, lib=host_lib)):
        assert list(got["donor"]) == [0, 6, 9] and list(got["hydrogen"]) == [1, 7, 10] and list(got["acceptor"]) == [0, 5, 6, 9, 12]
    none = script.hbond_sites_from_topology_native(pep, np.zeros((0, 2), np.int32), lib=host_lib)
    assert none["donor"].size == 0 and list(none["acceptor"]) == [0, 5, 6, 9, 12]
    with pytest.raises(script.ScriptError, match="names atoms"):
        script.hbond_sites_from_topology_native(pep, [(0, 13)], lib=host_lib)
    assert not host_lib.vmd_topology_hbond_sites(None, None, 0) and "NULL" in host_lib.last_error()


# ---- 8. the IR: every refusal, the fingerprint field by field, the statement next to the others ---------------------------------------------

def test_ir_validation_errors(host_lib):
    lib = host_lib
    for sym in ("vmd_ir_add_hbonds", "vmd_eval_hbonds", "vmd_eval_hbond_pairs", "vmd_topology_hbond_sites", "vmd_hbond_sites_view",
                "vmd_hbond_sites_free", "vmd_hip_sorted_atoms", "vmd_hip_hbond_atoms", "vmd_hip_hbond_brute", "vmd_hip_hbond_list",
                "vmd_hip_hbond_finish"):
        assert hasattr(lib, sym), sym
    ir = V.ScriptIR(lib)
    ok = dict(donors=[0, 0], hydrogens=[1, 2], acceptors=[0, 3], r_da=3.5, angle_min_deg=150.0)

    def bad(match, names=NAMES, **kw):
        with pytest.raises(V.VmdError, match=match):
            ir.add_hbonds(names, **dict(ok, **kw))
    bad("donor pair list is empty", donors=[], hydrogens=[])
    bad("acceptor list is empty", acceptors=[])
    bad("negative", donors=[0, -1])
    bad("negative", hydrogens=[1, -2])
    bad("negative", acceptors=[-3])
    bad("as donor and as its hydrogen", hydrogens=[1, 0])
    for r in (0.0, -1.0, float("inf"), float("nan")):
        bad("finite and positive", r_da=r)
    for a in (89.999, 180.001, -150.0, float("nan")):
        bad(r"\[90, 180\]", angle_min_deg=a)
    bad("name is empty", names=("", "occ"))
    bad("already defined", names=("x", "x"))
    names = (C.c_char_p * 2)(b"a", b"b")
    d, h, a = (np.array(v, np.int32) for v in ([0], [1], [2]))
    p = lambda x: x.ctypes.data_as(L.c_int32_p)
    sites = L.HbondSitesC(1, p(d), p(h), 1, p(a))
    assert not lib.vmd_ir_add_hbonds(None, names, C.byref(sites), 3.5, 150.0) and "ir is NULL" in lib.last_error()
    assert not lib.vmd_ir_add_hbonds(ir.h, None, C.byref(sites), 3.5, 150.0) and "two property names" in lib.last_error()
    assert not lib.vmd_ir_add_hbonds(ir.h, names, None, 3.5, 150.0) and "the sites" in lib.last_error()
    for s in (L.HbondSitesC(1, None, p(h), 1, p(a)), L.HbondSitesC(1, p(d), None, 1, p(a))):
        assert not lib.vmd_ir_add_hbonds(ir.h, names, C.byref(s), 3.5, 150.0) and "empty" in lib.last_error()
    assert not lib.vmd_ir_add_hbonds(ir.h, names, C.byref(L.HbondSitesC(1, p(d), p(h), 1, None)), 3.5, 150.0) and "empty" in lib.last_error()
    assert ir.property_count() == 0                                                # a refused statement leaves nothing behind
    ir.add_rmsd("g", [0, 1])
    bad("already defined", names=("g", "occ"))
    bad("already defined", names=("nhb", "g"))
    ir.add_hbonds(NAMES, **ok)
    for a in (90.0, 180.0):
        ir.add_hbonds((f"n{a:.0f}", f"o{a:.0f}"), **dict(ok, angle_min_deg=a))
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_rmsd("occ", [0, 1])
    assert ir.property_names()[:3] == ["g", "nhb", "occ"]
    assert ir.property_flags("nhb") == L.FLAG_TEMPORAL and ir.property_flags("occ") == L.FLAG_MAP
    ir2 = V.ScriptIR(lib)
    ir2.add_hbonds(NAMES, [0], [99], [2], 3.5, 150.0)
    if lib.vmd_device_count() > 0:
        cell = ((10.0, 10.0, 10.0), (0.0, 0.0, 0.0), 7)
        with pytest.raises(V.VmdError, match="references atom 99"):
            Run(lib, ir2, np.zeros((1, 3, 10), np.float32), cell)
        rn = Run(lib, ir, np.zeros((2, 3, 10), np.float32), cell)
        ev = rn.ev
        with pytest.raises(V.VmdError, match="not a hydrogen-bond occupancy"):
            ev.hbonds("nhb", 2)
        with pytest.raises(V.VmdError, match="not a hydrogen-bond property"):
            ev.hbond_pairs("g", rn.sysm, rn.traj, 0)
        with pytest.raises(V.VmdError, match="outside the trajectory"):
            ev.hbond_pairs("nhb", rn.sysm, rn.traj, 2)
        assert not lib.vmd_eval_hbonds(ev.h, b"nope", None, None, None) and "unknown property" in lib.last_error()
        assert not lib.vmd_eval_hbonds(None, b"occ", None, None, None) and "NULL" in lib.last_error()
        assert lib.vmd_eval_hbonds(ev.h, b"occ", None, None, None)                 # every output may be left out
        assert lib.vmd_eval_hbond_pairs(ev.h, b"nope", None, rn.traj.interface(), 0, None, 0) == C.c_size_t(-1).value
        assert lib.vmd_eval_hbond_pairs(None, b"occ", None, rn.traj.interface(), 0, None, 0) == C.c_size_t(-1).value
        assert lib.vmd_eval_hbond_pairs(ev.h, b"occ", None, rn.traj.interface(), 0, None, 0) == 0       # all atoms at the origin: uu == 0
        pd = ev.property_data("occ")
        assert pd.dim == (5, 1, 0, 0) and pd.unit_str == ("", "") and pd.hbond_accumulators.shape == (5,)
        assert list(pd.hbond_accumulators) == [0, 0, 0, 0, 2]
        assert ev.property_data("nhb").dim == (2, 1, 0, 0) and not rn.counts().any()
        assert ev.hbonds("occ")[2] == 2
        with pytest.raises(V.VmdError, match="occupancy record"):
            ev.export_table("/dev/null", "occ", "csv")


def test_fingerprint_work_and_atoms(host_lib):
    assert TR._old_ir(host_lib).fingerprint() == TR.PARENT_FINGERPRINT              # an IR without the forms keeps its fingerprint

    def fp(**kw):
        ir = V.ScriptIR(host_lib)
        a = dict(names=NAMES, donors=[0, 0, 3], hydrogens=[1, 2, 4], acceptors=[0, 3, 6], r_da=3.5, angle_min_deg=150.0)
        a.update(kw)
        ir.add_hbonds(**a)
        return ir.fingerprint(), int(host_lib.vmd_ir_work_per_frame(ir.h))
    f0, w0 = fp()
    variants = dict(name0=fp(names=("x", "occ")), name1=fp(names=("nhb", "x")), donor=fp(donors=[0, 0, 5]), hydrogen=fp(hydrogens=[1, 2, 5]),
                    acceptor=fp(acceptors=[0, 3, 7]), order=fp(acceptors=[3, 0, 6]), fewer=fp(acceptors=[0, 3]), r=fp(r_da=3.25),
                    angle=fp(angle_min_deg=120.0), pairs=fp(donors=[0, 0], hydrogens=[1, 2]))
    assert len({f0} | {v[0] for v in variants.values()}) == 1 + len(variants), variants
    assert w0 == 2 * 3 + 2 * 3 and variants["fewer"][1] == 2 * 3 + 2 * 2
    # a within count over the same lists is another statement (codes 14 / 15 against 8), and so is the walk's twin
    ir = V.ScriptIR(host_lib)
    ir.add_within_count("nhb", [0, 0, 3], [0, 3, 6], 0.0, 3.5)
    assert ir.fingerprint() != f0
    ir = TR._old_ir(host_lib)
    w_old = int(host_lib.vmd_ir_work_per_frame(ir.h))
    ir.add_hbonds(NAMES, [0, 0, 3], [1, 2, 4], [0, 3, 6], 3.5, 150.0)
    assert ir.fingerprint() != TR.PARENT_FINGERPRINT and int(host_lib.vmd_ir_work_per_frame(ir.h)) == w_old + 12
    assert list(ir.geometry_atoms("nhb")) == [0, 0, 3, 1, 2, 4, 0, 3, 6]             # donors, hydrogens, acceptors
    assert list(ir.geometry_atoms("nhb", 0)) == [0, 0, 3, 1, 2, 4, 0, 3, 6] and ir.geometry_atoms("nhb", 1).size == 0
    assert ir.geometry_atoms("occ").size == 0


def next_to_the_other_forms(lib, oracle, device=False):
    """VIAMD's default script plus rmsd, ramachandran, secondary_structure and rmsf statements, with and without an hbonds statement in the
    same IR: every other property is bit-identical, the new ones equal the restatement and an IR of their own"""
    atoms, blob, box, F = 6001, 200, 30.0, 6
    coords, topo = TG.blob_system(oracle, n_atoms=atoms, n_blob=blob, box=box, F=F, seed=5)
    names = np.array(["N", "CA", "C", "O", "CB", "H", "HA", "HB1", "CG", "HG"])
    topo.names = np.where(np.arange(atoms) < blob, names[np.arange(atoms) % 10], topo.elements)
    bb = script.backbone_from_topology(topo)
    o = script.backbone_oxygens_from_topology(topo, bb)
    el = np.array([str(e).upper() for e in topo.elements])
    wo = np.nonzero((el == "O") & (np.arange(atoms) >= blob))[0]
    bonds = [(int(i), int(i) + k) for i in wo for k in (1, 2) if i + k < atoms and el[i + k] == "H"]
    sites = script.hbond_sites_from_topology(topo, bonds)
    assert len(sites["donor"]) == len(bonds) > 1000 and len(sites["acceptor"]) >= len(wo)
    evs = []
    for with_hb in (False, True):
        ir = script.compile_script_native(TG.VIAMD_DEFAULT_SCRIPT + TR.RM_LINE, topo, lib=lib, **OPT_INS)
        ir.add_ramachandran(("bb", "rama"), **bb)
        ir.add_secondary_structure(("ss", "sspop"), bb["n"], bb["ca"], bb["c"], o, bb["range_offsets"], bb["rama_class"])
        ir.add_rmsf("fl", np.arange(blob, dtype=np.int32))
        if with_hb:
            ir.add_hbonds(NAMES, sites["donor"], sites["hydrogen"], sites["acceptor"], HC.R_DA, HC.ANGLE)
        evs.append(TG.evaluate(lib, ir, coords, box, topo.mass, device=device))
    plain, both = evs
    props = plain.ir.property_names()
    assert props == ["d1", "a1", "r", "v", "lin", "plan", "iso", "rm", "bb", "rama", "ss", "sspop", "fl"]
    assert both.ir.property_names() == props + list(NAMES)
    for name in props:
        a, b = plain.property_data(name), both.property_data(name)
        assert a.dim == b.dim and a.fingerprint == b.fingerprint, name
        assert np.array_equal(a.values.view(np.int32), b.values.view(np.int32)), name
        if a.c.counts:
            assert np.array_equal(a.counts, b.counts), name
    cell = ((box, box, box), (0.0, 0.0, 0.0), 7)
    want = restate(coords, cell, sites)
    print(f"blob system: {int(want['counts'].sum())} bonds, near the thresholds {want['near_d']} / {want['near_a']}")
    assert np.array_equal(TG.rows(both, NAMES[0])[:, 0].view(np.int32), want["counts"].view(np.int32))
    assert np.array_equal(both.property_data(NAMES[1]).hbond_accumulators, want["record"])
    alone = run(lib, sites, coords, cell, device)
    same((alone.counts(), alone.record()), (TG.rows(both, NAMES[0])[:, 0], both.property_data(NAMES[1]).hbond_accumulators), "an IR of its own")


def test_next_to_the_other_forms_on_the_emulator(emu_lib, oracle):
    next_to_the_other_forms(emu_lib, oracle)


def test_thresholds_were_exercised():
    """(runs last in this file: what the checks above counted near the thresholds, in one place)"""
    for what, (nd, na) in sorted(NEAR.items()):
        print(f"{what}: {nd} near r_da, {na} near the angle")
