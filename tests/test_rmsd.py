"""rmsd() on the emulator build and in the host-only entry points: known answers, bit parity with the pinned restatement and
the derived tolerance against the SVD one (tests/rmsd_ref.py), the reduction-order rule (call patterns), the pose's lifetime, ABI
validation, the opt-in script front-end (C++ and Python twin), multi-rank merges, export, and VIAMD's default script plus an rmsd line
through the shim with the three opt-ins."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import native_host

import viamd_amd as V
from viamd_amd import _lib as L
from viamd_amd import script, synth

import rmsd_ref as R
import test_geometry as TG
import test_shape as TS
from test_geometry import bits_equal, blob_system, evaluate, rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIAMD_DEFAULT_SCRIPT = TG.VIAMD_DEFAULT_SCRIPT
RM_LINE = '\nrm = rmsd(resname("ALA"));'


def check_tolerance(got, coords, box, sets, mass, what, geometric=False, frames=None, flags=7):
    """|got - ref| <= 2^-23 ref + min(delta / ref, sqrt(delta)), delta = max(n, 64) 2^-52 (Gp + Gq) / W (rmsd_ref.bound), against
    the SVD restatement, every value; bit-identity with the pinned restatement is counted and printed.  Returns that count."""
    got = np.asarray(got, np.float32)
    ref, bnd = R.values(coords, box, sets, mass, geometric=geometric, flags=flags, frames=frames, pinned=False, with_bound=True)
    pin = R.values(coords, box, sets, mass, geometric=geometric, flags=flags, frames=frames)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    off = int((got.view(np.int32) != pin.view(np.int32)).sum())
    diff = np.abs(got.astype(np.float64) - ref)
    ratio = np.where(diff == 0.0, 0.0, diff / np.maximum(bnd, 1e-300))
    print(f"{what}: {got.size} values, {off} not bit-identical to the pinned restatement, worst difference / bound {ratio.max():.3g}")
    assert (diff <= bnd).all(), f"{what}: {ratio.max():.3g} of the bound"
    return off


# ---- known answers -----------------------------------------------------------------------------------------------------------------

def two_frames(lib, p0, p1, box=32.0, mass=None, tilt=(0.0, 0.0, 0.0)):
    """frame 0 = the pose p0, frame 1 = p1 -> (both rows of rmsd(all points), coords)"""
    coords = np.stack([np.asarray(p0, np.float32).T, np.asarray(p1, np.float32).T]).copy()
    ir = V.ScriptIR(lib)
    ir.add_rmsd("g", list(range(coords.shape[2])))
    return rows(evaluate(lib, ir, coords, box, mass=mass, tilt=tilt), "g")[:, 0], coords


def scale_of(p, w=None):
    """(Gp + Gq) / W of a rigid copy: twice the weighted squared radius of gyration"""
    p = np.asarray(p, np.float64)
    w = np.ones(len(p)) if w is None else np.asarray(w, np.float64)
    c = (p * w[:, None]).sum(0) / w.sum()
    return 2.0 * float((w * ((p - c) ** 2).sum(1)).sum() / w.sum())


CHIRAL = np.array([(0, 0, 0), (1.5, 0, 0), (1.5, 2.25, 0), (1.5, 2.25, 3.125), (-0.5, 2.25, 3.125), (-0.5, 4, 3.125), (0.25, 4, 5),
                   (2, 4.5, 5.5), (2, 6, 4.75), (3.5, 6, 4.75), (3.5, 7.25, 6), (5, 7.25, 6.5)], np.float64)      # on a 2^-6 grid


def known_answers(lib):
    n = len(CHIRAL)
    # a rigidly rotated (quarter turns about z, then x) and translated copy that straddles the periodic faces of a cube of 32: every
    # coordinate is on a 2^-6 grid, so the fp32 copy is exact and the answer is 0 within sqrt(delta)
    p0 = CHIRAL + np.array([12.0, 10.0, 9.0])
    rot = np.stack([-CHIRAL[:, 1], CHIRAL[:, 0], CHIRAL[:, 2]], axis=1)              # (x, y, z) -> (-y, x, z)
    rot = np.stack([rot[:, 0], -rot[:, 2], rot[:, 1]], axis=1)                        # (x, y, z) -> (x, -z, y)
    p1 = np.mod(rot + np.array([3.0, 1.5, 30.25]), 32.0)
    assert (np.ptp(p1, axis=0) > 16.0).all()                                           # wrapped: it spans the cell on every axis
    got, coords = two_frames(lib, p0, p1)
    delta = max(n, 64) * 2.0 ** -52 * scale_of(CHIRAL)
    print(f"rigid copy: rmsd {got[1]:.3g}, sqrt(delta) {math.sqrt(delta):.3g}")
    assert got[0] == 0.0 and got.view(np.int32)[0] == 0                                # trajectory frame 0: +0, bit for bit
    assert 0.0 <= got[1] <= math.sqrt(delta)
    check_tolerance(got[:, None], coords, 32.0, list(range(n)), None, "rigid copy")
    # the same through a tilted cell
    got_t, coords_t = two_frames(lib, p0, p1, box=(32.0, 32.0, 32.0), tilt=(8.0, -4.0, 16.0))
    check_tolerance(got_t[:, None], coords_t, (32.0, 32.0, 32.0, 8.0, -4.0, 16.0), list(range(n)), None, "rigid copy, tilted cell")
    # without a cell the raw coordinates count: the wrapped copy is no rigid copy
    raw, _ = two_frames(lib, p0, p1, box=None)
    assert raw[1] > 1.0
    # two equal-mass atoms 3 apart in frame 0 and 5 later: each moved by 1
    got, _ = two_frames(lib, [(10, 10, 10), (13, 10, 10)], [(20, 5, 7), (20, 5, 12)])
    assert got[1] == 1.0 and got.view(np.int32)[0] == 0
    # a pose scaled by 1 + s about its centre of mass: s times the mass-weighted radius of gyration
    m = np.array([1, 12, 14, 16, 1, 1, 12, 12, 16, 14, 1, 32], np.float32)
    s = 0.25
    com = (CHIRAL * m[:, None]).sum(0) / m.sum()
    got, coords = two_frames(lib, CHIRAL + 8.0, com + (1 + s) * (CHIRAL - com) + 8.0, mass=m)
    want = s * math.sqrt(scale_of(CHIRAL, m) / 2.0)
    assert abs(got[1] - want) <= R.bound(want, (1 + (1 + s) ** 2) * scale_of(CHIRAL, m) / 2.0, n) + 2.0 ** -22 * want   # (+ the fp32 coordinates)
    check_tolerance(got[:, None], coords, 32.0, list(range(n)), m, "scaled pose")
    # a mirror image: Horn's method fits a proper rotation, so the value is the determinant-corrected Kabsch one and exceeds the
    # improper fit's (0)
    mirror = CHIRAL * np.array([1.0, 1.0, -1.0]) + 8.0
    got, coords = two_frames(lib, CHIRAL + 8.0, mirror)
    check_tolerance(got[:, None], coords, 32.0, list(range(n)), None, "mirror image")
    assert got[1] > 0.5
    # degenerate sets: finite, never NaN
    for what, pts in (("one atom", [(3, 4, 5)]), ("coincident", [(3, 4, 5)] * 5), ("collinear", [(1, 1, 1), (2, 2, 2), (4, 4, 4), (7, 7, 7)]),
                      ("planar", [(0, 0, 2), (3, 0, 2), (3, 4, 2), (0, 4, 2), (1, 1, 2)])):
        later = [(2 * x + 1, y + 0.5 * z, z - 1) for x, y, z in pts]
        got, coords = two_frames(lib, pts, later)
        assert np.isfinite(got).all() and got.view(np.int32)[0] == 0, what
        if what in ("one atom", "coincident"):
            assert got[1] == 0.0, what
        check_tolerance(got[:, None], coords, 32.0, list(range(len(pts))), None, what)
    # unequal masses pull the value; spec_dist_geometric_com ignores them
    bent = CHIRAL.copy()
    bent[-1] += (0.0, 0.0, 3.0)                                                          # the heavy atom is the one that moved
    plain, _ = two_frames(lib, CHIRAL + 8.0, bent + 8.0)
    weighted, coords = two_frames(lib, CHIRAL + 8.0, bent + 8.0, mass=m)
    assert weighted[1] > plain[1] > 0.0
    assert bits_equal(weighted, R.values(coords, 32.0, list(range(n)), m)[:, 0])
    old = lib.vmd_set_option(b"spec_dist_geometric_com", 1)
    try:
        assert bits_equal(two_frames(lib, CHIRAL + 8.0, bent + 8.0, mass=m)[0], plain)
    finally:
        lib.vmd_set_option(b"spec_dist_geometric_com", old)
    # flags, unit, shape of the record: as distance has them
    ir = V.ScriptIR(lib)
    ir.add_rmsd("g", [0, 1, 2])
    assert ir.property_flags("g") == L.FLAG_TEMPORAL
    pd = evaluate(lib, ir, coords, 32.0).property_data("g")
    assert pd.unit_str == ("", "Å") and tuple(pd.dim[:2]) == (2, 1)


def chain_system(n=3000, cells=5, L=20.0, F=3, seed=11):
    """a random-walk chain `cells` cells wide that tumbles: frame f is frame 0 under an arbitrary rotation and translation plus 0.1 A of
    noise, wrapped into the cell.  -> (coords float32 [F, 3, n], the unwrapped fp64 frames)"""
    rng = np.random.default_rng(seed)
    step = rng.normal(0.0, 0.6, (n, 3)) + np.array([cells * L / n, 0.3 * cells * L / n, 0.0])
    base = np.cumsum(step, axis=0)
    whole = [base]
    for f in range(1, F):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                        [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                        [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        whole.append(base @ rot.T + rng.uniform(-50, 50, 3) + rng.normal(0.0, 0.1, (n, 3)))
    coords = np.stack([np.mod(p, L).T for p in whole]).astype(np.float32)
    coords[coords >= L] = 0.0
    return coords, whole


def kabsch(p, q):
    """unweighted RMSD of two whole fp64 point sets after the best proper rotation (SVD)"""
    p, q = p - p.mean(0), q - q.mean(0)
    U, _, Vt = np.linalg.svd(p.T @ q)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    return math.sqrt((((p @ U @ D @ Vt) - q) ** 2).sum() / len(p))


def wide_chain(lib):
    coords, whole = chain_system()
    assert np.ptp(whole[0][:, 0]) > 4.5 * 20.0
    ir = V.ScriptIR(lib)
    idx = np.arange(coords.shape[2], dtype=np.int32)
    ir.add_rmsd("g", idx)
    got = rows(evaluate(lib, ir, coords, 20.0), "g")
    check_tolerance(got, coords, 20.0, idx, None, "chain 5 cells wide under rotation")
    for f in (1, 2):
        want = kabsch(whole[f], whole[0])                      # from the coordinates before wrapping and rounding to fp32
        print(f"chain frame {f}: {got[f, 0]:.6f} against {want:.6f} from the whole fp64 chain")
        assert 0.05 < want < 0.3 and abs(got[f, 0] - want) < 1e-4       # fp32 coordinates in a 20 A cell: 1e-6 A each


def test_known_answers_on_the_emulator(emu_lib):
    known_answers(emu_lib)


def test_a_wide_chain_that_tumbles_on_the_emulator(emu_lib):
    wide_chain(emu_lib)


# ---- parity with the references --------------------------------------------------------------------------------------------------------

CELLS = [((30.0, 30.0, 30.0), (0.0, 0.0, 0.0)), ((24.0, 22.0, 20.0), (5.0, -3.0, 4.0))]
OPEN_CELLS = TS.OPEN_CELLS          # a slab with y open, a wire along y: links longer than half a cell that take no shift
# 63: one idle lane in the butterfly and the wave scan; 64 / 65: wave-per-set kernel / block kernels; 255 / 256 / 257: thread 0 takes a
# second atom (the second s_tot slot); CHUNK +- 1, 2 CHUNK - 1: the chunk seams - the link across and the carried-in shift, a last chunk
# of one atom included; the last: three chunks
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 2 * R.CHUNK - 1, 2 * R.CHUNK + 808]
POPULATIONS = [[1, 3, 64, 65, 200, R.CHUNK + 5, 700], [1, 2, 3, 10, 64, 33], [10, 64, 700, R.CHUNK + 5]]
COPIES = TS.COPIES


def random_system(seed, n_atoms, F=3):
    rng = np.random.default_rng(seed)
    # an anisotropic cloud that spills over the periodic faces: the chain through it crosses cells at nearly every link
    coords = (rng.uniform(-6, 36, (F, 3, n_atoms)) * np.array([1.0, 0.5, 0.2])[None, :, None]).astype(np.float32)
    return rng, coords, rng.uniform(1, 16, n_atoms).astype(np.float32)


def size_sweep(lib, box, tilt=(0.0, 0.0, 0.0), flags=7, exact=True, device=False, sizes=SIZES, populations=POPULATIONS):
    """Single sets of the edge sizes, unequal populations, the alone / small-population / next-to-large identity and the equal columns,
    in one cell.  exact (the emulator): bit-identical to the pinned restatement.  Every value within rmsd_ref.bound of the SVD
    restatement; the values not bit-identical to the pinned one are counted and printed.  Row 0 is +0 bit for bit.  device: a resident
    trajectory, which must give the bits of the host-staged one.  A partly periodic cell (flags != 7) must change the restatement's
    own numbers."""
    rng, coords, mass = random_system(1, 9100)
    bx = tuple(box) + tuple(tilt)
    tag = f"tilt {tilt}, flags {flags}"

    def run(sets):
        ir = V.ScriptIR(lib)
        ir.add_rmsd_population("g", sets)
        got = rows(evaluate(lib, ir, coords, box, mass, tilt=tilt, flags=flags, device=device), "g")
        assert got.shape == (3, len(sets)) and not got.view(np.int32)[0].any()                      # trajectory frame 0: +0
        if device:
            assert bits_equal(got, rows(evaluate(lib, ir, coords, box, mass, tilt=tilt, flags=flags), "g")), "resident / host-staged"
        return got

    for n in sizes:
        idx = rng.choice(9100, n, replace=False).astype(np.int32)
        ir = V.ScriptIR(lib)
        ir.add_rmsd("g", idx)
        got = rows(evaluate(lib, ir, coords, box, mass, tilt=tilt, flags=flags, device=device), "g")
        assert got.shape == (3, 1) and not got.view(np.int32)[0].any()
        if device:
            assert bits_equal(got, rows(evaluate(lib, ir, coords, box, mass, tilt=tilt, flags=flags), "g")), "resident / host-staged"
        off = check_tolerance(got, coords, bx, idx, mass, f"{n} atoms, {tag}", flags=flags)
        assert not exact or off == 0, n
        if flags != 7 and n >= 63:
            assert not bits_equal(R.values(coords, bx, idx, mass, flags=flags), R.values(coords, bx, idx, mass)), \
                f"{n} atoms: the open axes change nothing"
    for sizes_p in populations:
        sets = [rng.choice(9100, n, replace=False).astype(np.int32) for n in sizes_p]
        off = check_tolerance(run(sets), coords, bx, sets, mass, f"population {sizes_p}, {tag}", flags=flags)
        assert not exact or off == 0, sizes_p
    # a set gives the same bits alone, in a population of small sets and in a population with a large one
    small = rng.choice(9100, 40, replace=False).astype(np.int32)
    big = rng.choice(9100, 5000, replace=False).astype(np.int32)
    res = [run(sets)[:, pos] for sets, pos in (([small], 0), ([small, small[:7]], 0), ([big, small], 1))]
    assert bits_equal(res[0], res[1]) and bits_equal(res[0], res[2]) and res[0][1] > 0.0
    # P columns of that set: bit-equal, whichever wave of whichever block forms them
    for P in COPIES:
        got = run([small] * P)
        for c in range(P):
            assert bits_equal(got[:, c], res[0]), (P, c)


@pytest.mark.parametrize("box,tilt", CELLS)
def test_emulator_matches_the_pinned_reference_bit_for_bit(emu_lib, box, tilt):
    size_sweep(emu_lib, box, tilt)


@pytest.mark.parametrize("box,flags", OPEN_CELLS)
def test_emulator_matches_the_pinned_reference_in_partly_periodic_cells(emu_lib, box, flags):
    size_sweep(emu_lib, box, flags=flags)


# ---- half-cell ties ------------------------------------------------------------------------------------------------------------------

def half_cell_ties(lib, box, flags=7, exact=True, device=False):
    """TS.tie_system along the chain: every third link is exactly L / 2, -L / 2, 3 L / 2 or -3 L / 2 long on one axis.  Frame 0 is the
    pose; frame 1 holds the same points in reverse order (every link negated: the ties round the other way) and frame 2 a rigidly moved
    copy (the same links from other coordinates)."""
    pose, sets = TS.tie_system(box, chain=True)
    rev = pose.copy()
    for s in sets:
        rev[0][:, s] = pose[0][:, s[::-1]]
    moved = pose + np.array([7.25, -11.5, 2.125], np.float32)[None, :, None]
    coords = np.concatenate([pose, rev, moved]).astype(np.float32)
    x = coords.astype(np.float64)
    Lf = np.asarray(box, np.float32).astype(np.float64)
    if float(np.float32(box[0])) == box[0]:                     # the ties are exact: d / L is a half-integer, bit for bit, in every frame
        for f in range(3):
            q = np.concatenate([np.diff(x[f][:, s], axis=1) / Lf[:, None] for s in sets], axis=1)
            assert ((np.abs(q) == 0.5).sum(axis=1) >= 6).all() and ((np.abs(q) == 1.5).sum(axis=1) >= 6).all(), f
    mass = np.random.default_rng(32).uniform(1, 16, coords.shape[2]).astype(np.float32)
    for group, what in ((sets[:3], "ties, one wave per set"), (sets[3:] + sets[:1], "ties, block kernels")):
        ir = V.ScriptIR(lib)
        ir.add_rmsd_population("g", group)
        got = rows(evaluate(lib, ir, coords, box, mass, flags=flags, device=device), "g")
        assert not got.view(np.int32)[0].any()
        off = check_tolerance(got, coords, box, group, mass, f"{what}, cell {box}, flags {flags}", flags=flags)
        assert not exact or off == 0, (what, box, flags)
        if flags != 7:          # the open axis takes no shift however long the link is: the periodic cell's numbers differ
            assert not bits_equal(R.values(coords, box, group, mass, flags=flags), R.values(coords, box, group, mass))


@pytest.mark.parametrize("box,flags", TS.TIE_CELLS)
def test_half_cell_ties_on_the_emulator(emu_lib, box, flags):
    half_cell_ties(emu_lib, box, flags)


POP_SCRIPT = ('g = rmsd(all);\nga = rmsd(resname("ALA"));\ngr = rmsd(all) in resname("ALA");\n'
              "gw = rmsd(element('O')) in residue(15:60);")


def script_populations(lib, coords, topo, box, tilt=(0.0, 0.0, 0.0), geometric=0, what="blob"):
    """the config 4-style blob: every frame of the four forms against both restatements -> values not bit-identical to the pinned one"""
    old = lib.vmd_set_option(b"spec_dist_geometric_com", geometric)
    try:
        ir, info = script.compile_script(POP_SCRIPT, topo, lib=lib, rmsd=True)
        ev = evaluate(lib, ir, coords, box, topo.mass, tilt=tilt)
        off = 0
        for name in ("g", "ga", "gr", "gw"):
            sets = info[name]["sets"]
            assert info[name]["kind"] == "rmsd"
            got = rows(ev, name)
            assert got.shape == (coords.shape[0], len(sets))
            off += check_tolerance(got, coords, tuple(box) + tuple(tilt) if tilt != (0.0, 0.0, 0.0) else box, sets, topo.mass,
                                   f"{what} {name} geometric={geometric} tilt={tilt}", geometric=bool(geometric))
            assert not got[0].any() and not got.view(np.int32)[0].any()                    # trajectory frame 0: +0
        assert len(info["g"]["sets"]) == 1 and info["g"]["sets"][0].size == topo.num_atoms
        assert len(info["ga"]["sets"]) == 1 and info["ga"]["sets"][0].size == 200
        assert [s.size for s in info["gr"]["sets"]] == [10] * 20                           # inside a context `all` is the context's atoms
        assert len(info["gw"]["sets"]) == 46 and all(s.size == 1 for s in info["gw"]["sets"])     # one oxygen per residue: 0, never NaN
        assert not rows(ev, "gw").any() and rows(ev, "ga")[1:].min() > 0.0
        return off
    finally:
        lib.vmd_set_option(b"spec_dist_geometric_com", old)


@pytest.mark.parametrize("geometric", [0, 1])
def test_script_populations_on_the_emulator(emu_lib, oracle, geometric):
    coords, topo = blob_system(oracle)
    assert script_populations(emu_lib, coords, topo, (30.0, 30.0, 30.0), geometric=geometric) == 0
    assert script_populations(emu_lib, coords, topo, (30.0, 30.0, 30.0), tilt=(6.0, -3.0, 9.0), geometric=geometric) == 0


# ---- the reduction-order rule: call patterns ----------------------------------------------------------------------------------------

CALL_SCRIPT = 'g = rmsd(all); gr = rmsd(all) in resname("ALA"); gb = rmsd(resname("ALA")); d = distance(10, 30);'
CALL_NAMES = ("g", "gr", "gb", "d")
RAGGED = [(0, 7), (7, 8), (8, 31), (31, 60)]
LATE_FIRST = [(31, 60), (7, 8), (8, 31), (0, 7)]           # the ranges that do not hold trajectory frame 0 come first


def call_patterns(lib, run):
    """run(ranges=None, pooled=None) -> eval; every pattern must give the bits of the single call"""
    one = run()
    variants = {"16 pool threads, grain 1": dict(pooled=(16, 1)), "4 pool threads, grain 5": dict(pooled=(4, 5)),
                "ragged ranges": dict(ranges=RAGGED), "ranges without frame 0 first": dict(ranges=LATE_FIRST)}
    got = {k: run(**kw) for k, kw in variants.items()}
    for bf in (3, 16):
        old = lib.vmd_set_option(b"batch_frames", bf)
        try:
            got[f"batch_frames {bf}"] = run()
            got[f"batch_frames {bf}, late first"] = run(ranges=LATE_FIRST)
        finally:
            lib.vmd_set_option(b"batch_frames", old)
    for what, ev in got.items():
        assert ev.frame_mask().all(), what
        for name in CALL_NAMES:
            assert bits_equal(rows(ev, name), rows(one, name)), (what, name)
    for name in CALL_NAMES[:3]:
        r = rows(one, name)
        assert not r.view(np.int32)[0].any() and (r[1:] > 0.0).all(), name
    return one


def test_call_patterns_are_bit_identical(emu_lib, oracle):
    coords, topo = blob_system(oracle, n_atoms=5200, n_blob=200, F=60)       # `all`: two chunks
    ir = script.compile_script(CALL_SCRIPT, topo, lib=emu_lib, rmsd=True)[0]
    one = call_patterns(emu_lib, lambda **kw: evaluate(emu_lib, ir, coords, 30.0, topo.mass, **kw))
    agg = one.property_data("gr").aggregate
    r = rows(one, "gr")
    np.testing.assert_allclose(agg["mean"], r.mean(axis=1), rtol=1e-5, atol=1e-6)       # population aggregates: arithmetic, as for distances
    np.testing.assert_array_equal(agg["ext"][:, 1], r.max(axis=1))


def test_interrupt_and_clear(emu_lib, oracle):
    coords, topo = blob_system(oracle, F=9)
    ir = script.compile_script(CALL_SCRIPT, topo, lib=emu_lib, rmsd=True)[0]
    one = evaluate(emu_lib, ir, coords, 30.0, topo.mass)
    cell = V.make_unitcell(30.0)
    ev = V.ScriptEval(coords.shape[0], ir)
    sysm, traj = V.MolSystem(coords.shape[2], mass=topo.mass, unitcell=cell), V.HostTrajectory(coords, cell)
    ev.interrupt()
    ev.frame_range(sysm, traj, 0, coords.shape[0])
    ev.clear_data()
    assert not ev.frame_mask().any() and not rows(ev, "g").any()
    assert ev.frame_range(sysm, traj, 0, coords.shape[0])
    for name in CALL_NAMES:
        assert bits_equal(rows(ev, name), rows(one, name))


def pose_lifetime(lib, coords_a, coords_b, topo, box=30.0):
    """the pose belongs to (evaluator, trajectory): one evaluator over A and then over B equals a fresh evaluator on B"""
    ir = script.compile_script(CALL_SCRIPT, topo, lib=lib, rmsd=True)[0]
    fresh = evaluate(lib, ir, coords_b, box, topo.mass)
    cell = V.make_unitcell(box)
    F = coords_a.shape[0]
    sysm = V.MolSystem(coords_a.shape[2], mass=topo.mass, unitcell=cell)
    traj_a, traj_b = V.HostTrajectory(coords_a, cell), V.HostTrajectory(coords_b, cell)      # both alive: two identities
    ev = V.ScriptEval(F, ir)
    assert ev.frame_range(sysm, traj_a, 0, F)
    on_a = {n: rows(ev, n) for n in CALL_NAMES}
    ev.clear_data()
    assert ev.frame_range(sysm, traj_b, 2, F) and ev.frame_range(sysm, traj_b, 0, 2)          # B's frame 0 is not in the first range
    for name in CALL_NAMES:
        assert bits_equal(rows(ev, name), rows(fresh, name)), name
    assert not bits_equal(on_a["g"], rows(fresh, "g"))
    ev.clear_data()
    assert ev.frame_range(sysm, traj_a, 0, F)                                                   # and back again
    for name in CALL_NAMES:
        assert bits_equal(rows(ev, name), on_a[name]), name


def test_pose_lifetime(emu_lib, oracle):
    coords_a, topo = blob_system(oracle, F=6)
    coords_b, _ = blob_system(oracle, F=6, seed=9)
    pose_lifetime(emu_lib, coords_a, coords_b, topo)


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------

def test_ir_validation_errors(host_lib):
    lib = host_lib
    for sym in ("vmd_ir_add_rmsd", "vmd_ir_add_rmsd_population", "vmd_hip_rmsd", "vmd_hip_rmsd_pose", "vmd_hip_rmsd_workspace_bytes"):
        assert hasattr(lib, sym), sym
    ir = V.ScriptIR(lib)
    with pytest.raises(V.VmdError, match="empty"):
        ir.add_rmsd("g", [])
    with pytest.raises(V.VmdError, match="negative"):
        ir.add_rmsd("g", [0, -1])
    with pytest.raises(V.VmdError, match="empty"):
        ir.add_rmsd_population("g", [[0], []])                                     # offsets that do not increase
    with pytest.raises(V.VmdError, match="name is empty"):
        ir.add_rmsd("", [0, 1])
    a = np.array([0, 1], np.int32)
    p = lambda x: x.ctypes.data_as(L.c_int32_p)
    assert not lib.vmd_ir_add_rmsd_population(ir.h, b"x", 2, p(a), p(np.array([1, 2, 3], np.int32)))
    assert "start at 0" in lib.last_error()
    assert not lib.vmd_ir_add_rmsd_population(ir.h, b"x", 0, p(a), p(np.array([0, 1, 2], np.int32)))
    assert "empty" in lib.last_error()
    assert not lib.vmd_ir_add_rmsd_population(ir.h, b"x", 1, p(a), None)
    assert "offsets" in lib.last_error()
    assert not lib.vmd_ir_add_rmsd(ir.h, None, p(a), 2)
    assert "name is empty" in lib.last_error()
    assert ir.property_count() == 0                                                # a refused statement leaves nothing behind
    ir.add_distance("g", [0], [1])
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_rmsd("g", [0, 1])
    ir.add_rmsd("g2", [0, 1])
    assert ir.property_names() == ["g", "g2"] and ir.property_flags("g2") == L.FLAG_TEMPORAL
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_distance("g2", [0], [1])
    # the distance entry points keep refusing kinds above 3 (7 is the rmsd descriptor's own)
    for kind in (4, 6, 7):
        assert not lib.vmd_ir_add_distance(ir.h, b"k", kind, p(a), 2, p(a), 2) and "unknown distance kind" in lib.last_error()
        off = np.array([0, 2], np.int32)
        assert not lib.vmd_ir_add_distance_population(ir.h, b"k", kind, 1, p(a), p(off), p(a), p(off))
        assert "unknown distance kind" in lib.last_error()
    assert lib.vmd_hip_rmsd_workspace_bytes(10, 3, 64) == 10 * 3 * 14 * 8            # one wave per set: the sums only
    assert lib.vmd_hip_rmsd_workspace_bytes(0, 3, 64) == 0
    assert lib.vmd_hip_rmsd_workspace_bytes(10, 3, 65) == 10 * 3 * 1 * (14 * 8 + 16)
    assert lib.vmd_hip_rmsd_workspace_bytes(2, 1, 2 * R.CHUNK + 1) == 2 * 3 * (14 * 8 + 16)
    ir2 = V.ScriptIR(lib)
    ir2.add_rmsd("g", [0, 99])
    if lib.vmd_device_count() > 0:
        with pytest.raises(V.VmdError, match="references atom 99"):
            evaluate(lib, ir2, np.zeros((1, 3, 10), np.float32), 10.0)


# fingerprint of the IR built by _old_ir, taken with the library of the parent commit (before rmsd existed): an IR without an rmsd
# property keeps it
PARENT_FINGERPRINT = 0x3E193418FFD37220


def _old_ir(lib):
    ir = V.ScriptIR(lib)
    ir.add_rdf("r", [0, 1, 2], [3, 4], (0.5, 9.0))
    ir.add_distance("d", [0, 1], [2])
    ir.add_distance_population("dp", [[0], [1, 2]], [[3], [4]], L.DIST_MIN)
    ir.add_angle_population("a", [[0], [1, 2]], [[3], [4]], [[5, 6, 7], [8]])
    ir.add_dihedral("t", [0], [1], [2], [3, 4])
    ir.add_shape_weights(("lin", "plan", "iso"), [0, 1, 2, 3])
    return ir


def test_fingerprint_work_and_atoms(host_lib):
    assert _old_ir(host_lib).fingerprint() == PARENT_FINGERPRINT

    def fp(build):
        ir = V.ScriptIR(host_lib)
        build(ir)
        return ir.fingerprint(), int(host_lib.vmd_ir_work_per_frame(ir.h))
    f0, w0 = fp(lambda ir: ir.add_rmsd("g", [0, 1, 2, 3]))
    f_name, _ = fp(lambda ir: ir.add_rmsd("h", [0, 1, 2, 3]))
    f_set, _ = fp(lambda ir: ir.add_rmsd("g", [0, 1, 2, 4]))
    f_order, _ = fp(lambda ir: ir.add_rmsd("g", [0, 2, 1, 3]))                 # the chain runs in the order given
    f_pop, w_pop = fp(lambda ir: ir.add_rmsd_population("g", [[0, 1], [2, 3]]))
    f_pop2, w_pop2 = fp(lambda ir: ir.add_rmsd_population("g", [[0, 1, 2], [3], [4, 5, 6, 7]]))
    f_dist, _ = fp(lambda ir: ir.add_distance("g", [0, 1, 2, 3], [0]))
    f_shape, _ = fp(lambda ir: ir.add_shape_weights(("g", "p", "i"), [0, 1, 2, 3]))
    assert len({f0, f_name, f_set, f_order, f_pop, f_pop2, f_dist, f_shape}) == 8
    assert (w0, w_pop, w_pop2) == (4, 4, 8)                  # the atoms of every context's set
    ir = _old_ir(host_lib)
    w_old = int(host_lib.vmd_ir_work_per_frame(ir.h))
    ir.add_rmsd_population("g", [[0, 1, 2], [3], [4, 5, 6, 7]])
    assert ir.fingerprint() != PARENT_FINGERPRINT and int(host_lib.vmd_ir_work_per_frame(ir.h)) == w_old + 8
    assert list(ir.geometry_atoms("g")) == [0, 1, 2, 3, 4, 5, 6, 7]
    assert list(ir.geometry_atoms("g", 2)) == [4, 5, 6, 7] and list(ir.geometry_atoms("g", 1)) == [3]
    assert ir.geometry_atoms("g", 3).size == 0 and ir.geometry_atoms("d").size == 0


# ---- front-end -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def topo():
    return synth.water_box_topology(200 + 933 * 3, n_blob=200)


REASON_OFF = "unsupported function 'rmsd' (outside the rdf / sdf / distance path)"        # the parent commit's words


def test_without_the_opt_in_rmsd_is_reported_as_ever(host_lib, topo):
    text = VIAMD_DEFAULT_SCRIPT + RM_LINE
    ir_a, rep_a = script.compile_script_native(text, topo, lib=host_lib, partial=True, angles=True, shape=True)
    ir_b, rep_b = script.compile_script_native(text, topo, lib=host_lib, partial=True, angles=True, shape=True, rmsd=False)
    ir_py, _, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, angles=True, shape=True, rmsd=False)
    assert ir_a.property_names() == ir_b.property_names() == ir_py.property_names() == ["d1", "a1", "r", "v", "lin", "plan", "iso"]
    assert ir_a.fingerprint() == ir_b.fingerprint() == ir_py.fingerprint()
    assert rep_a == rep_b == rep_py
    assert [k["names"] for k in rep_a["skipped"]] == ["rm"] and rep_a["skipped"][0]["reason"] == REASON_OFF
    k = rep_a["skipped"][0]
    assert text[k["beg"]:k["end"]] == RM_LINE[1:-1]
    assert len(rep_a["fallback_source"]) == len(text) and rep_a["fallback_source"].strip().endswith(RM_LINE[1:])
    # the script without the line compiles to the fingerprint it has always had, whatever the new bit says
    ir_0 = script.compile_script_native(VIAMD_DEFAULT_SCRIPT, topo, lib=host_lib, angles=True, shape=True)
    ir_1 = script.compile_script_native(VIAMD_DEFAULT_SCRIPT, topo, lib=host_lib, angles=True, shape=True, rmsd=True)
    ir_2 = script.compile_script(VIAMD_DEFAULT_SCRIPT, topo, lib=host_lib, angles=True, shape=True, rmsd=True)[0]
    assert ir_0.fingerprint() == ir_1.fingerprint() == ir_2.fingerprint() == ir_a.fingerprint()
    for compiler in (script.compile_script_native, script.compile_script):
        with pytest.raises(script.ScriptError) as err:
            compiler("rm = rmsd(all);", topo, lib=host_lib, angles=True, shape=True)
        assert str(err.value) == REASON_OFF
        with pytest.raises(script.ScriptError, match="unsupported function 'rmsd'"):
            compiler("{a,b,c} = rmsd(all);", topo, lib=host_lib, angles=True, shape=True)


def test_default_script_with_the_three_opt_ins(host_lib, topo):
    text = VIAMD_DEFAULT_SCRIPT + RM_LINE
    ir_c, rep_c = script.compile_script_native(text, topo, lib=host_lib, partial=True, angles=True, shape=True, rmsd=True)
    ir_py, info, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, angles=True, shape=True, rmsd=True)
    assert ir_c.property_names() == ir_py.property_names() == ["d1", "a1", "r", "v", "lin", "plan", "iso", "rm"]
    assert ir_c.fingerprint() == ir_py.fingerprint() and ir_c.property_flags("rm") == L.FLAG_TEMPORAL
    assert rep_c == rep_py and rep_c["skipped"] == []
    fb = rep_c["fallback_source"]
    assert len(fb) == len(text) and fb.strip() == 's1 = resname("ALA")[2:8];' and fb.count("\n") == text.count("\n")
    assert info["rm"]["kind"] == "rmsd" and list(info["rm"]["sets"][0]) == list(range(200)) == list(ir_c.geometry_atoms("rm"))
    strict_c = script.compile_script_native(text, topo, lib=host_lib, angles=True, shape=True, rmsd=True)
    strict_py = script.compile_script(text, topo, lib=host_lib, angles=True, shape=True, rmsd=True)[0]
    assert strict_c.fingerprint() == strict_py.fingerprint() == ir_c.fingerprint()
    # the bit alone: the two other statements are the ones left
    ir_s, rep_s = script.compile_script_native(text, topo, lib=host_lib, partial=True, rmsd=True)
    ir_sp, _, rep_sp = script.compile_script(text, topo, lib=host_lib, partial=True, rmsd=True)
    assert ir_s.property_names() == ir_sp.property_names() == ["d1", "r", "v", "rm"]
    assert rep_s == rep_sp and [k["names"] for k in rep_s["skipped"]] == ["a1", "lin,plan,iso"] and ir_s.fingerprint() == ir_sp.fingerprint()
    # a skipped statement that uses the name keeps the rmsd statement in the fallback's text
    ir_k, rep_k = script.compile_script_native(text + "\nx = rm * 2;", topo, lib=host_lib, partial=True, angles=True, shape=True, rmsd=True)
    ir_kp, _, rep_kp = script.compile_script(text + "\nx = rm * 2;", topo, lib=host_lib, partial=True, angles=True, shape=True, rmsd=True)
    assert rep_k == rep_kp and [k["names"] for k in rep_k["skipped"]] == ["x"]
    assert RM_LINE[1:] in rep_k["fallback_source"] and "shape_weights" not in rep_k["fallback_source"]
    assert ir_k.property_names() == ir_kp.property_names() == ir_c.property_names()


BAD_STATEMENTS = [
    ("rm = rmsd(all, water);", "rm", "rm: rmsd takes one selection"),
    ('rm = rmsd(resname("XYZ"));', "rm", "rm: empty selection"),
    ('rm = rmsd(element(\'N\')) in resname("HOH");', "rm", "rm: empty selection inside a context"),
    ("rm = rmsd(all) in element('O');", "rm", "rm: `in` needs an array of structures"),
    ("{a,b,c} = rmsd(all);", "a,b,c", "a,b,c: rmsd defines one property, not a tuple"),
    ("rm = rmsd();", "rm", ""),
    ("rm = rmsd(all;", "rm", "rm: missing ')'"),
    ("d = rmsd(all);", "d", "already defined"),
]


@pytest.mark.parametrize("stmt,names,reason", BAD_STATEMENTS)
def test_malformed_statements(host_lib, topo, stmt, names, reason):
    text = "d = distance(1, 2);\n" + stmt + "\ne = distance(3, 4);"
    for compiler in (script.compile_script_native, script.compile_script):
        with pytest.raises((script.ScriptError, V.VmdError)) as err:        # (the twin passes a descriptor the library refuses on as VmdError)
            compiler(text, topo, lib=host_lib, rmsd=True)
        assert reason in str(err.value)
    if "(all;" in stmt:
        return                                                              # (an open parenthesis swallows the rest of the script)
    ir_c, rep_c = script.compile_script_native(text, topo, lib=host_lib, partial=True, rmsd=True)
    ir_py, _, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, rmsd=True)
    assert ir_c.property_names() == ir_py.property_names() == ["d", "e"] and ir_c.fingerprint() == ir_py.fingerprint()
    assert rep_c == rep_py and len(rep_c["skipped"]) == 1
    k = rep_c["skipped"][0]
    assert k["names"] == names and reason in k["reason"] and text[k["beg"]:k["end"]] == stmt[:-1]
    assert stmt in rep_c["fallback_source"] and "distance(3, 4)" not in rep_c["fallback_source"]


def test_forms_the_twins_agree_on(host_lib, topo):
    t = script.Topology(topo.elements, topo.resnames, topo.residue_index, mass=topo.mass, residue_seq_id=topo.residue_index + 101)
    for form, P in (('a = rmsd(protein);', 1), ('a = rmsd(all) in residue(4);', 1), ('a = rmsd(all) in resid(104:110);', 7),
                    ('a = rmsd(element(\'H\')) in resname("HOH");', 933),
                    ('s = resname("ALA")[2:8]; a = rmsd(s); e = rmsd(all) in s;', None)):
        ir_c = script.compile_script_native(form, t, lib=host_lib, rmsd=True)
        ir_py, info = script.compile_script(form, t, lib=host_lib, rmsd=True)
        assert ir_c.property_names() == ir_py.property_names() and ir_c.fingerprint() == ir_py.fingerprint(), form
        if P is not None:
            assert len(info["a"]["sets"]) == P
        else:
            assert len(info["a"]["sets"]) == 1 and info["a"]["sets"][0].size == 70 and [s.size for s in info["e"]["sets"]] == [10] * 7


# ---- multi-rank ------------------------------------------------------------------------------------------------------------------------

MERGE_SCRIPT = 'g = rmsd(all); gr = rmsd(all) in resname("ALA"); d = distance(10, 30);'
MERGE_NAMES = ("g", "gr", "d")


def _merge_worker(rank, world, port, tmpdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import conftest
    from viamd_amd.dist import reduce_eval, shard_frames
    from oracle import oracle as O
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lib = V.VmdLib(conftest.EMU_LIB)
    coords, topo = blob_system(O, F=7)
    ir = script.compile_script(MERGE_SCRIPT, topo, lib=lib, rmsd=True)[0]
    F = coords.shape[0]
    ev = V.ScriptEval(F, ir)
    beg, end = shard_frames(F, rank, world)
    assert (beg == 0) == (rank == 0)                  # only rank 0 holds trajectory frame 0; the others fetch it for the pose
    cell = V.make_unitcell(30.0)
    assert ev.frame_range(V.MolSystem(coords.shape[2], mass=topo.mass, unitcell=cell), V.HostTrajectory(coords, cell), beg, end)
    reduce_eval(ev)
    assert ev.frame_mask().all()
    out = {n: ev.property_data(n).values for n in MERGE_NAMES}
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), mean=ev.property_data("gr").aggregate["mean"], **out)
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_multi_rank_merge(emu_lib, oracle, tmp_path, world):
    import torch.multiprocessing as mp
    port = 37500 + (os.getpid() % 2000) + 7 * world
    mp.spawn(_merge_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    coords, topo = blob_system(oracle, F=7)
    ir = script.compile_script(MERGE_SCRIPT, topo, lib=emu_lib, rmsd=True)[0]
    one = evaluate(emu_lib, ir, coords, 30.0, topo.mass)
    for r in range(world):
        z = np.load(tmp_path / f"rank{r}.npz")
        for n in MERGE_NAMES:
            assert bits_equal(z[n].reshape(7, -1), rows(one, n)), n
        assert bits_equal(z["mean"], one.property_data("gr").aggregate["mean"])


def test_export_table(emu_lib, oracle, tmp_path):
    coords, topo = blob_system(oracle, F=5)
    ir = script.compile_script('rm = rmsd(resname("ALA"));', topo, lib=emu_lib, rmsd=True)[0]
    ev = evaluate(emu_lib, ir, coords, 30.0, topo.mass)
    y = rows(ev, "rm")[:, 0]
    for ext in ("xvg", "csv"):
        path = tmp_path / f"rm.{ext}"
        ev.export_table(path, "rm", ext)
        text = open(path, encoding="utf-8").read()
        assert "rm" in text, text[:400]
        nums = [ln.replace(",", " ").split() for ln in text.splitlines() if ln.strip() and ln.strip()[0] in "0123456789"]
        assert len(nums) == 5
        np.testing.assert_allclose(np.array([float(ln[1]) for ln in nums], np.float32), y, rtol=1e-5, atol=2e-6)   # six decimals in the file


# ---- VIAMD's default script plus the rmsd line through the shim ------------------------------------------------------------------------

def build_shim_rmsd():
    """tests/native/shim_default_script_rmsd.cpp linked against the product library"""
    return native_host.build_shim("shim_default_script_rmsd")


def test_shim_default_script_with_the_rmsd_line_on_the_emulator(emu_lib, tmp_path):
    import conftest
    exe = native_host.build_shim("shim_default_script_rmsd", conftest.build_emu(), tmp_path / "shim_rmsd_emu")
    native_host.run_ok([exe, "8"], "OK frames=8 properties=8 rm=gpu fallback_frame_range_calls=0")
    # without the RMSD bit `rm` is reported and stays with the (mock) fallback, which is driven over the frames again
    out = native_host.run_ok([exe, "8", "nobit"], "OK frames=8 properties=8 rm=fallback")
    assert "fallback_frame_range_calls=0" not in out.stdout, out.stdout
