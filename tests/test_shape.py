"""shape_weights() on the emulator build and in the host-only entry points: known answers, bit parity with the pinned
restatement and the absolute tolerance against the plain one (tests/shape_ref.py), the reduction-order rule (call patterns), one
computation per statement, ABI validation, the opt-in script front-end (C++ and Python twin), VIAMD's call pattern (interrupt /
clear_data, multi-rank merges), export, and VIAMD's default script through the shim with both opt-ins."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import native_host

import viamd_amd as V
from viamd_amd import _lib as L
from viamd_amd import script, synth

import shape_ref as S
import test_geometry as TG
from test_geometry import bits_equal, blob_system, evaluate, rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lin", "plan", "iso")
VIAMD_DEFAULT_SCRIPT = TG.VIAMD_DEFAULT_SCRIPT


def weights(ev, names=NAMES):
    """float32 [3, F, P]"""
    return np.stack([rows(ev, n) for n in names])


def check_tolerance(got, ref, what):
    """|got - ref| <= 2^-23, absolute, every value (both sides carry fp64 errors far below fp32 resolution, then each rounds
    once to fp32 - at most half an ulp of a value in [0, 1], 2^-24, on either side).  Never a ulp count: the small weights of a rod or a
    plane differ by millions of ulps while agreeing to 1e-16."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    off = int((got.view(np.int32) != ref.view(np.int32)).sum())
    worst = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    print(f"{what}: {got.size} values, {off} not bit-identical, worst absolute difference {worst:.3g}")
    assert np.isfinite(got).all(), what
    assert worst <= S.TOL, f"{what}: {worst:.3g} from the reference"


# ---- known answers -----------------------------------------------------------------------------------------------------------------

def one_frame(lib, pts, box=50.0, mass=None):
    xyz = np.asarray(pts, np.float32).T.copy()[None]
    ir = V.ScriptIR(lib)
    ir.add_shape_weights(NAMES, list(range(xyz.shape[2])))
    return tuple(float(v) for v in weights(evaluate(lib, ir, xyz, box, mass=mass))[:, 0, 0])


def known_answers(lib):
    assert one_frame(lib, [(0, 0, 0), (1, 0, 0), (2, 0, 0), (5, 0, 0)]) == (1.0, 0.0, 0.0)                       # atoms on a line
    assert one_frame(lib, [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)]) == (0.0, 1.0, 0.0)                       # corners of a square
    assert one_frame(lib, [(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]) == (0.0, 0.0, 1.0)       # ... of a cube
    assert one_frame(lib, [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]) == (0.0, 0.0, 1.0)   # octahedron
    assert one_frame(lib, [(3, 4, 5)]) == (0.0, 0.0, 0.0)                                                       # one atom: 0, 0, 0, never NaN
    assert one_frame(lib, [(3, 4, 5)] * 5) == (0.0, 0.0, 0.0)                                                   # coincident atoms
    # a set straddling the periodic faces of a cube of 20 equals its unwrapped copy and the copy shifted into the middle of the cell
    straddling = [(19, 1, 10), (1, 2, 10), (0.5, 19, 9), (2, 3, 11)]
    unwrapped = [(-1, 1, 10), (1, 2, 10), (0.5, -1, 9), (2, 3, 11)]
    middle = [(x + 10, y + 10, z) for x, y, z in unwrapped]
    a, b, c = (one_frame(lib, p, box=20.0) for p in (straddling, unwrapped, middle))
    assert a == b == c and abs(sum(a) - 1.0) < 3e-7 and min(a) > 0.0
    assert one_frame(lib, straddling, box=None) != a                                                             # no cell: the raw coordinates
    # unequal masses pull the measures; spec_dist_geometric_com ignores them
    ell = [(0, 0, 0), (4, 0, 0), (0, 1, 0), (0, 0, 0.5)]
    heavy = np.array([1, 1, 1, 12], np.float32)
    plain, weighted = one_frame(lib, ell), one_frame(lib, ell, mass=heavy)
    assert plain != weighted
    old = lib.vmd_set_option(b"spec_dist_geometric_com", 1)
    try:
        assert one_frame(lib, ell, mass=heavy) == plain
    finally:
        lib.vmd_set_option(b"spec_dist_geometric_com", old)
    xyz = np.asarray(ell, np.float32).T.copy()[None]
    assert bits_equal(np.array(weighted, np.float32), S.values(xyz, 50.0, [0, 1, 2, 3], heavy)[:, 0, 0])
    ir = V.ScriptIR(lib)
    ir.add_shape_weights(("a", "b", "c"), [0, 1, 2])
    assert [ir.property_flags(n) for n in "abc"] == [L.FLAG_TEMPORAL] * 3
    ev = evaluate(lib, ir, xyz, 50.0)
    pd = ev.property_data("b")
    assert pd.unit_str == ("", "") and tuple(pd.dim[:2]) == (1, 1)


def test_known_answers_on_the_emulator(emu_lib):
    known_answers(emu_lib)


# ---- parity with the references --------------------------------------------------------------------------------------------------------

CELLS = [((30.0, 30.0, 30.0), (0.0, 0.0, 0.0)), ((24.0, 22.0, 20.0), (5.0, -3.0, 4.0))]
# partly periodic orthorhombic cells (box, periodic-axis bits): a slab with y open, a wire along y (x and z open).  random_system's
# cloud is 42 wide in x and 21 in y, so with these cells every set of 63 atoms or more has offsets beyond half of Lx or Ly that the open
# axis must leave alone.  (z open alone changes nothing - the cloud's z extent never exceeds half a cell - so it is not used.)
OPEN_CELLS = [((30.0, 12.0, 30.0), 5), ((30.0, 14.0, 26.0), 2)]
# 63: one idle lane in the butterfly; 64 / 65: wave-per-set kernel / block kernels; 255 / 256 / 257: thread 0 takes a second atom;
# CHUNK +- 1, 2 CHUNK - 1: the chunk seams (a last chunk of one atom included); the last: three chunks
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, S.CHUNK - 1, S.CHUNK, S.CHUNK + 1, 2 * S.CHUNK - 1, 2 * S.CHUNK + 808]
# unequal sets: the largest beyond one chunk (blocks per chunk, contexts with fewer chunks than the largest) / of at most 64 atoms (one wave
# per set) / the large set last
POPULATIONS = [[1, 3, 64, 65, 200, S.CHUNK + 5, 700], [1, 2, 3, 10, 64, 33], [10, 64, 700, S.CHUNK + 5]]
COPIES = (1, 4, 5, 64, 65)        # columns of one set: the partial last block of k_*_small, the partial last wave of k_*_finish


def random_system(seed, n_atoms, F=2):
    rng = np.random.default_rng(seed)
    # an anisotropic cloud that spills over the periodic faces
    coords = (rng.uniform(-6, 36, (F, 3, n_atoms)) * np.array([1.0, 0.5, 0.2])[None, :, None]).astype(np.float32)
    return rng, coords, rng.uniform(1, 16, n_atoms).astype(np.float32)


def size_sweep(lib, box, tilt=(0.0, 0.0, 0.0), flags=7, exact=True, device=False, sizes=SIZES, populations=POPULATIONS):
    """Single sets of the edge sizes, unequal populations, the alone / small-population / next-to-large identity and the equal columns,
    in one cell.  exact (the emulator): bit-identical to the pinned restatement.  Every value within S.TOL of both restatements; the
    values not bit-identical to the pinned one are counted and printed.  device: a resident trajectory, which must give the bits of
    the host-staged one.  A partly periodic cell (flags != 7) must change the restatement's own numbers."""
    rng, coords, mass = random_system(1, 9100)
    bx = tuple(box) + tuple(tilt)
    tag = f"tilt {tilt}, flags {flags}"

    def run(build):
        ir = V.ScriptIR(lib)
        build(ir)
        got = weights(evaluate(lib, ir, coords, box, mass, tilt=tilt, flags=flags, device=device))
        if device:
            assert bits_equal(got, weights(evaluate(lib, ir, coords, box, mass, tilt=tilt, flags=flags))), "resident / host-staged"
        return got

    def check(got, sets, what):
        pin = S.values(coords, bx, sets, mass, flags=flags)
        if exact:
            assert bits_equal(got, pin), what
        check_tolerance(got, pin, f"{what}, {tag} / pinned")
        check_tolerance(got, S.values(coords, bx, sets, mass, flags=flags, pinned=False), f"{what}, {tag} / plain")
        return pin

    for n in sizes:
        idx = rng.choice(9100, n, replace=False).astype(np.int32)
        pin = check(run(lambda ir: ir.add_shape_weights(NAMES, idx)), idx, f"{n} atoms")
        if flags != 7 and n >= 63:
            assert not bits_equal(pin, S.values(coords, bx, idx, mass)), f"{n} atoms: the open axes change nothing"
    for sizes_p in populations:
        sets = [rng.choice(9100, n, replace=False).astype(np.int32) for n in sizes_p]
        got = run(lambda ir: ir.add_shape_weights_population(NAMES, sets))
        assert got.shape == (3, 2, len(sizes_p))
        check(got, sets, f"population {sizes_p}")
    # a set gives the same bits alone, in a population of small sets and in a population with a large one
    small = rng.choice(9100, 40, replace=False).astype(np.int32)
    big = rng.choice(9100, 5000, replace=False).astype(np.int32)
    res = []
    for sets, pos in (([small], 0), ([small, small[:7]], 0), ([big, small], 1)):
        res.append(run(lambda ir: ir.add_shape_weights_population(NAMES, sets))[:, :, pos])
    assert bits_equal(res[0], res[1]) and bits_equal(res[0], res[2])
    # P columns of that set: bit-equal, whichever wave of whichever block forms them
    for P in COPIES:
        got = run(lambda ir: ir.add_shape_weights_population(NAMES, [small] * P))
        assert got.shape == (3, 2, P)
        for c in range(P):
            assert bits_equal(got[:, :, c], res[0]), (P, c)


@pytest.mark.parametrize("box,tilt", CELLS)
def test_emulator_matches_the_pinned_reference_bit_for_bit(emu_lib, box, tilt):
    size_sweep(emu_lib, box, tilt)


@pytest.mark.parametrize("box,flags", OPEN_CELLS)
def test_emulator_matches_the_pinned_reference_in_partly_periodic_cells(emu_lib, box, flags):
    size_sweep(emu_lib, box, flags=flags)


# ---- half-cell ties ------------------------------------------------------------------------------------------------------------------

TIE_STEPS = (0.5, -0.5, 1.5, -1.5)
# (cell, periodic-axis bits): 1 / 20 ... are inexact in fp64 for 30 and 100 (d * (1 / L) falls beside the half-integer: the division
# decides); 24.7f is no fp32-exact half (the near-tie, not the tie); one cell with a different L per axis; a slab with y open and a
# wire along y, where the open axes must take no shift from atoms 3 L / 2 away.  49: with those cells fl(d * fl(1 / L)) happens to land
# on the half-integer itself, so rint of it already agrees with the quotient's; 73.5 * fl(1 / 49) is 1.5 - 2^-52, which rounds to 1
# where the tie goes to 2 - the cell at which the result depends on the division branch
TIE_CELLS = [((20.0, 20.0, 20.0), 7), ((30.0, 30.0, 30.0), 7), ((100.0, 100.0, 100.0), 7), ((24.7, 24.7, 24.7), 7),
             ((20.0, 30.0, 100.0), 7), ((30.0, 30.0, 30.0), 5), ((30.0, 30.0, 30.0), 2), ((49.0, 49.0, 49.0), 7)]
assert np.rint(73.5 * (1.0 / 49.0)) == 1.0 and np.rint(73.5 / 49.0) == 2.0
TIE_SIZES = (5, 23, 64, 70)          # three sets for the wave-per-set kernels, one for the block kernels


def tie_system(box, sizes=TIE_SIZES, chain=False, seed=31):
    """-> (float32 [1, 3, N], the index sets).  Every set starts at (3, 4, 5).  Every third atom lies exactly L / 2, -L / 2, 3 L / 2 or
    -3 L / 2 (fp32 arithmetic on the fp32 cell) along one axis from the set's first atom - chain=True: from its predecessor in the
    set - and off by an ordinary amount along the others; the rest are ordinary.  Ordinary offsets are on a 2^-8 grid, so with
    L / 2 on that grid every sum is exact in fp32.  Not collinear, not planar."""
    rng = np.random.default_rng(seed)
    L = np.asarray(box, np.float32)
    pts, sets = [], []
    for n in sizes:
        first = len(pts)
        p = [np.array([3.0, 4.0, 5.0], np.float32)]
        for j in range(1, n):
            ordinary = (rng.integers(-640, 641, 3) / np.float32(256.0)).astype(np.float32)       # |offset| <= 2.5
            if chain:
                ordinary = ordinary * np.float32(0.5)
            if j % 3 == 1:
                axis, step = (j // 3) % 3, np.float32(TIE_STEPS[(j // 9) % 4])
                ordinary[axis] = step * L[axis]
            p.append(((p[-1] if chain else p[0]) + ordinary).astype(np.float32))
        pts.extend(p)
        sets.append(np.arange(first, first + n, dtype=np.int32))
    return np.asarray(pts, np.float32).T.copy()[None], sets


def half_cell_ties(lib, box, flags=7, exact=True, device=False):
    coords, sets = tie_system(box)
    x = coords[0].astype(np.float64)
    Lf = np.asarray(box, np.float32).astype(np.float64)
    if float(np.float32(box[0])) == box[0]:                     # the ties are exact: d / L is a half-integer, bit for bit
        q = np.concatenate([(x[:, s] - x[:, s[:1]]) / Lf[:, None] for s in sets], axis=1)
        assert ((np.abs(q) == 0.5).sum(axis=1) >= 6).all() and ((np.abs(q) == 1.5).sum(axis=1) >= 6).all()
    mass = np.random.default_rng(32).uniform(1, 16, coords.shape[2]).astype(np.float32)
    for group, what in ((sets[:3], "ties, one wave per set"), (sets[3:] + sets[:1], "ties, block kernels")):
        ir = V.ScriptIR(lib)
        ir.add_shape_weights_population(NAMES, group)
        got = weights(evaluate(lib, ir, coords, box, mass, flags=flags, device=device))
        pin = S.values(coords, box, group, mass, flags=flags)
        if exact:
            assert bits_equal(got, pin), (what, box, flags)
        check_tolerance(got, pin, f"{what}, cell {box}, flags {flags} / pinned")
        check_tolerance(got, S.values(coords, box, group, mass, flags=flags, pinned=False), f"{what}, cell {box}, flags {flags} / plain")
        assert min(v.min() for v in pin[:, 0, [k for k, g in enumerate(group) if g.size > 5]]) > 1e-3          # no rod, no plane
        if flags != 7:          # the open axis takes no shift however far the atom is: the periodic cell's numbers differ
            assert not bits_equal(pin, S.values(coords, box, group, mass))


@pytest.mark.parametrize("box,flags", TIE_CELLS)
def test_half_cell_ties_on_the_emulator(emu_lib, box, flags):
    half_cell_ties(emu_lib, box, flags)


@pytest.mark.parametrize("geometric", [0, 1])
def test_script_populations_on_the_emulator(emu_lib, oracle, geometric):
    coords, topo = blob_system(oracle)
    old = emu_lib.vmd_set_option(b"spec_dist_geometric_com", geometric)
    try:
        src = ('{l,p,i} = shape_weights(all);\n{la,pa,ia} = shape_weights(resname("ALA"));\n'
               '{lr,pr,ir} = shape_weights(all) in resname("ALA");\n{lw,pw,iw} = shape_weights(element(\'O\')) in residue(15:60);')
        ir, info = script.compile_script(src, topo, lib=emu_lib, shape=True)
        ev = evaluate(emu_lib, ir, coords, 30.0, topo.mass)
        for names in (("l", "p", "i"), ("la", "pa", "ia"), ("lr", "pr", "ir"), ("lw", "pw", "iw")):
            sets = info[names[0]]["sets"]
            assert [info[n]["component"] for n in names] == [0, 1, 2] and info[names[2]]["sets"] is sets
            got = weights(ev, names)
            assert got.shape[2] == len(sets)
            assert bits_equal(got, S.values(coords, 30.0, sets, topo.mass, geometric=geometric)), names
            check_tolerance(got, S.values(coords, 30.0, sets, topo.mass, geometric=geometric, pinned=False), f"{names} geometric={geometric}")
        assert len(info["l"]["sets"]) == 1 and info["l"]["sets"][0].size == 1200
        assert len(info["la"]["sets"]) == 1 and info["la"]["sets"][0].size == 200
        assert [s.size for s in info["lr"]["sets"]] == [10] * 20                # inside a context `all` is the context's atoms
        assert len(info["lw"]["sets"]) == 46 and all(s.size == 1 for s in info["lw"]["sets"])      # one oxygen per residue: 0, 0, 0
        assert not weights(ev, ("lw", "pw", "iw")).any()
    finally:
        emu_lib.vmd_set_option(b"spec_dist_geometric_com", old)


# ---- the reduction-order rule: call patterns ----------------------------------------------------------------------------------------

CALL_SCRIPT = '{l,p,i} = shape_weights(all); {lr,pr,ir} = shape_weights(all) in resname("ALA"); {lb,pb,ib} = shape_weights(resname("ALA"));'
CALL_NAMES = ("l", "p", "i", "lr", "pr", "ir", "lb", "pb", "ib")
RAGGED = [(0, 7), (7, 8), (8, 31), (31, 60)]


def call_patterns(lib, run):
    """run(ranges=None, pooled=None) -> eval; every pattern must give the bits of the single call"""
    one = run()
    variants = {"16 pool threads, grain 1": dict(pooled=(16, 1)), "ragged ranges": dict(ranges=RAGGED)}
    got = {k: run(**kw) for k, kw in variants.items()}
    for bf in (3, 16):
        old = lib.vmd_set_option(b"batch_frames", bf)
        try:
            got[f"batch_frames {bf}"] = run()
        finally:
            lib.vmd_set_option(b"batch_frames", old)
    for what, ev in got.items():
        for name in CALL_NAMES:
            assert bits_equal(rows(ev, name), rows(one, name)), (what, name)
    return one


def test_call_patterns_are_bit_identical(emu_lib, oracle):
    coords, topo = blob_system(oracle, n_atoms=5200, n_blob=200, F=60)       # `all`: two chunks
    ir = script.compile_script(CALL_SCRIPT, topo, lib=emu_lib, shape=True)[0]
    one = call_patterns(emu_lib, lambda **kw: evaluate(emu_lib, ir, coords, 30.0, topo.mass, **kw))
    agg = one.property_data("pr").aggregate
    r = rows(one, "pr")
    np.testing.assert_allclose(agg["mean"], r.mean(axis=1), rtol=1e-5, atol=1e-6)       # population aggregates: arithmetic, as for distances
    np.testing.assert_array_equal(agg["ext"][:, 0], r.min(axis=1))


# ---- one computation per statement ----------------------------------------------------------------------------------------------------

def launch_counts(lib, make_eval, read):
    """launches booked under "shape" and "distance" while the eval runs and `read` names are fetched"""
    lib.vmd_profile_reset()
    lib.vmd_profile_enable(True)
    try:
        ev = make_eval()
        for n in read:
            ev.property_data(n)
    finally:
        lib.vmd_profile_enable(False)
    out = []
    for key in (b"shape", b"distance"):
        n = C.c_uint64(0)
        lib.vmd_profile_ms(key, C.byref(n))
        out.append(int(n.value))
    return out


def one_computation_per_statement(lib, coords, topo, box):
    ir = script.compile_script('d = distance(1, 2); {l,p,i} = shape_weights(all);', topo, lib=lib, shape=True)[0]
    F = coords.shape[0]
    old = lib.vmd_set_option(b"batch_frames", 5)
    try:
        one = launch_counts(lib, lambda: evaluate(lib, ir, coords, box, topo.mass), ["i"])
        all3 = launch_counts(lib, lambda: evaluate(lib, ir, coords, box, topo.mass), ["l", "p", "i"])
    finally:
        lib.vmd_set_option(b"batch_frames", old)
    batches = (F + 4) // 5
    assert one == all3 == [batches, batches], (one, all3)        # per statement and batch - as often as the one distance statement


def test_one_computation_per_statement(emu_lib, oracle):
    coords, topo = blob_system(oracle, F=18)
    one_computation_per_statement(emu_lib, coords, topo, 30.0)


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------

def test_ir_validation_errors(host_lib):
    lib = host_lib
    ir = V.ScriptIR(lib)
    with pytest.raises(V.VmdError, match="empty"):
        ir.add_shape_weights(NAMES, [])
    with pytest.raises(V.VmdError, match="negative"):
        ir.add_shape_weights(NAMES, [0, -1])
    with pytest.raises(V.VmdError, match="empty"):
        ir.add_shape_weights_population(NAMES, [[0], []])                          # offsets that do not increase
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_shape_weights(("a", "b", "a"), [0, 1])                              # a name twice in one statement
    with pytest.raises(V.VmdError, match="name is empty"):
        ir.add_shape_weights(("a", "", "c"), [0, 1])
    a = np.array([0, 1], np.int32)
    p = lambda x: x.ctypes.data_as(L.c_int32_p)
    names = (C.c_char_p * 3)(b"x", b"y", b"z")
    assert not lib.vmd_ir_add_shape_weights_population(ir.h, names, 2, p(a), p(np.array([1, 2, 3], np.int32)))
    assert "start at 0" in lib.last_error()
    assert not lib.vmd_ir_add_shape_weights_population(ir.h, names, 0, p(a), p(np.array([0, 1, 2], np.int32)))
    assert "empty" in lib.last_error()
    assert not lib.vmd_ir_add_shape_weights(ir.h, None, p(a), 2)
    assert "three property names" in lib.last_error()
    assert ir.property_count() == 0                                                # a refused statement leaves none of its names behind
    ir.add_distance("lin", [0], [1])
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_shape_weights(NAMES, [0, 1])                                        # clashes with an earlier property
    assert ir.property_names() == ["lin"]
    ir.add_shape_weights(("l2", "p2", "i2"), [0, 1])
    assert ir.property_names() == ["lin", "l2", "p2", "i2"]
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_distance("p2", [0], [1])
    ir2 = V.ScriptIR(lib)
    ir2.add_shape_weights(NAMES, [0, 99])
    if lib.vmd_device_count() > 0:
        with pytest.raises(V.VmdError, match="references atom 99"):
            evaluate(lib, ir2, np.zeros((1, 3, 10), np.float32), 10.0)


# fingerprint of the IR built by _old_ir on the parent commit (before shape_weights existed): an IR without shape properties keeps it
PARENT_FINGERPRINT = 0x4E212B8F7C856C8C


def _old_ir(lib):
    ir = V.ScriptIR(lib)
    ir.add_rdf("r", [0, 1, 2], [3, 4], (0.5, 9.0))
    ir.add_distance("d", [0, 1], [2])
    ir.add_distance_population("dp", [[0], [1, 2]], [[3], [4]], L.DIST_MIN)
    ir.add_angle_population("a", [[0], [1, 2]], [[3], [4]], [[5, 6, 7], [8]])
    ir.add_dihedral("t", [0], [1], [2], [3, 4])
    return ir


def test_fingerprint_work_and_atoms(host_lib):
    assert _old_ir(host_lib).fingerprint() == PARENT_FINGERPRINT

    def fp(build):
        ir = V.ScriptIR(host_lib)
        build(ir)
        return ir.fingerprint(), int(host_lib.vmd_ir_work_per_frame(ir.h))
    f0, w0 = fp(lambda ir: ir.add_shape_weights(NAMES, [0, 1, 2, 3]))
    f_names, _ = fp(lambda ir: ir.add_shape_weights(("lin", "plan", "isx"), [0, 1, 2, 3]))
    f_order, _ = fp(lambda ir: ir.add_shape_weights(("plan", "lin", "iso"), [0, 1, 2, 3]))
    f_set, _ = fp(lambda ir: ir.add_shape_weights(NAMES, [0, 1, 2, 4]))
    f_pop, w_pop = fp(lambda ir: ir.add_shape_weights_population(NAMES, [[0, 1], [2, 3]]))
    f_pop2, w_pop2 = fp(lambda ir: ir.add_shape_weights_population(NAMES, [[0, 1, 2], [3], [4, 5, 6, 7]]))
    f_dist, _ = fp(lambda ir: [ir.add_distance(n, [0, 1, 2, 3], [0]) for n in NAMES])
    assert len({f0, f_names, f_order, f_set, f_pop, f_pop2, f_dist}) == 7
    assert (w0, w_pop, w_pop2) == (4, 4, 8)                  # the atoms of every context's set, once per statement
    ir = _old_ir(host_lib)
    w_old = int(host_lib.vmd_ir_work_per_frame(ir.h))
    ir.add_shape_weights_population(NAMES, [[0, 1, 2], [3], [4, 5, 6, 7]])
    assert ir.fingerprint() != PARENT_FINGERPRINT and int(host_lib.vmd_ir_work_per_frame(ir.h)) == w_old + 8
    for n in NAMES:
        assert list(ir.geometry_atoms(n)) == [0, 1, 2, 3, 4, 5, 6, 7]
        assert list(ir.geometry_atoms(n, 2)) == [4, 5, 6, 7] and list(ir.geometry_atoms(n, 1)) == [3]
        assert ir.geometry_atoms(n, 3).size == 0
    assert ir.geometry_atoms("d").size == 0


# ---- front-end -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def topo():
    return synth.water_box_topology(200 + 933 * 3, n_blob=200)


def test_default_script_without_the_shape_opt_in_is_unchanged(host_lib, topo):
    """what tests/test_geometry.py::test_default_script_with_the_opt_in expects today, from every entry point that can say `shape off`"""
    text = VIAMD_DEFAULT_SCRIPT
    ir_a, rep_a = script.compile_script_native(text, topo, lib=host_lib, partial=True, angles=True)
    ir_b, rep_b = script.compile_script_native(text, topo, lib=host_lib, partial=True, angles=True, shape=False)
    ir_py, _, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, angles=True, shape=False)
    assert ir_a.property_names() == ir_b.property_names() == ir_py.property_names() == ["d1", "a1", "r", "v"]
    assert ir_a.fingerprint() == ir_b.fingerprint() == ir_py.fingerprint()
    assert rep_a == rep_b == rep_py
    assert [k["names"] for k in rep_a["skipped"]] == ["lin,plan,iso"]
    assert rep_a["skipped"][0]["reason"] == "unsupported function 'shape_weights' (outside the rdf / sdf / distance path)"
    fb = rep_a["fallback_source"]
    assert len(fb) == len(text) and "angle" not in fb and "{lin,plan,iso} = shape_weights(all);" in fb
    # neither opt-in: d1, r, v and both statements reported, as ever
    ir_0, rep_0 = script.compile_script_native(text, topo, lib=host_lib, partial=True)
    assert ir_0.property_names() == ["d1", "r", "v"] and [k["names"] for k in rep_0["skipped"]] == ["a1", "lin,plan,iso"]
    with pytest.raises(script.ScriptError, match="unsupported function 'shape_weights'"):
        script.compile_script_native("{a,b,c} = shape_weights(all);", topo, lib=host_lib, angles=True)
    with pytest.raises(script.ScriptError, match="unsupported function 'shape_weights'"):
        script.compile_script("{a,b,c} = shape_weights(all);", topo, lib=host_lib, angles=True)


def test_default_script_with_both_opt_ins(host_lib, topo):
    text = VIAMD_DEFAULT_SCRIPT
    ir_c, rep_c = script.compile_script_native(text, topo, lib=host_lib, partial=True, angles=True, shape=True)
    ir_py, info, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, angles=True, shape=True)
    assert ir_c.property_names() == ir_py.property_names() == ["d1", "a1", "r", "v", "lin", "plan", "iso"]
    assert ir_c.fingerprint() == ir_py.fingerprint()
    assert [ir_c.property_flags(n) for n in NAMES] == [L.FLAG_TEMPORAL] * 3
    assert rep_c == rep_py and rep_c["skipped"] == []
    fb = rep_c["fallback_source"]
    assert len(fb) == len(text) and fb.strip() == 's1 = resname("ALA")[2:8];'            # every property statement blanked
    assert fb.count("\n") == text.count("\n")
    assert info["lin"]["sets"][0].size == topo.num_atoms and list(ir_c.geometry_atoms("iso")) == list(range(topo.num_atoms))
    # the strict form takes the whole script now
    strict_c = script.compile_script_native(text, topo, lib=host_lib, angles=True, shape=True)
    strict_py = script.compile_script(text, topo, lib=host_lib, angles=True, shape=True)[0]
    assert strict_c.fingerprint() == strict_py.fingerprint() == ir_c.fingerprint()
    # shape alone: the angle statement is the one left
    ir_s, rep_s = script.compile_script_native(text, topo, lib=host_lib, partial=True, shape=True)
    ir_sp, _, rep_sp = script.compile_script(text, topo, lib=host_lib, partial=True, shape=True)
    assert ir_s.property_names() == ir_sp.property_names() == ["d1", "r", "v", "lin", "plan", "iso"]
    assert rep_s == rep_sp and [k["names"] for k in rep_s["skipped"]] == ["a1"] and ir_s.fingerprint() == ir_sp.fingerprint()
    # a skipped statement that uses one of the three names keeps the shape statement in the fallback's text
    ir_k, rep_k = script.compile_script_native(text + "\nx = plan * 2;", topo, lib=host_lib, partial=True, angles=True, shape=True)
    ir_kp, _, rep_kp = script.compile_script(text + "\nx = plan * 2;", topo, lib=host_lib, partial=True, angles=True, shape=True)
    assert rep_k == rep_kp and [k["names"] for k in rep_k["skipped"]] == ["x"]
    assert "{lin,plan,iso} = shape_weights(all);" in rep_k["fallback_source"] and "angle" not in rep_k["fallback_source"]
    assert ir_k.property_names() == ir_kp.property_names() == ["d1", "a1", "r", "v", "lin", "plan", "iso"]


BAD_STATEMENTS = [
    ("{a,b} = shape_weights(all);", "a,b", "a,b: shape_weights defines three properties"),
    ("{a,b,c,d} = shape_weights(all);", "a,b,c,d", "a,b,c,d: shape_weights defines three properties"),
    ("a = shape_weights(all);", "a", "a: shape_weights defines three properties"),
    ("{a,b,c} = shape_weights(all, water);", "a,b,c", "a,b,c: shape_weights takes one selection"),
    ('{a,b,c} = shape_weights(resname("XYZ"));', "a,b,c", "a,b,c: empty selection"),
    ('{a,b,c} = shape_weights(element(\'N\')) in resname("HOH");', "a,b,c", "a,b,c: empty selection inside a context"),
    ("{a,b,c} = shape_weights(all) in element('O');", "a,b,c", "a,b,c: `in` needs an array of structures"),
    ("{a,b,a} = shape_weights(all);", "a,b,a", "already defined"),
    ("{a,b,c} = distance(1, 2);", "a,b,c", "unsupported function 'distance'"),            # any other tuple assignment: as today
]


@pytest.mark.parametrize("stmt,names,reason", BAD_STATEMENTS)
def test_arity_and_argument_errors(host_lib, topo, stmt, names, reason):
    text = "d = distance(1, 2);\n" + stmt + "\ne = distance(3, 4);"
    for compiler in (script.compile_script_native, script.compile_script):
        with pytest.raises((script.ScriptError, V.VmdError)) as err:        # (the twin passes a descriptor the library refuses on as VmdError)
            compiler(text, topo, lib=host_lib, shape=True)
        assert reason in str(err.value)
    ir_c, rep_c = script.compile_script_native(text, topo, lib=host_lib, partial=True, shape=True)
    ir_py, _, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, shape=True)
    assert ir_c.property_names() == ir_py.property_names() == ["d", "e"] and ir_c.fingerprint() == ir_py.fingerprint()
    assert rep_c == rep_py and len(rep_c["skipped"]) == 1
    k = rep_c["skipped"][0]
    assert k["names"] == names and reason in k["reason"] and text[k["beg"]:k["end"]] == stmt[:-1]
    assert stmt in rep_c["fallback_source"] and "distance(3, 4)" not in rep_c["fallback_source"]


def test_forms_the_twins_agree_on(host_lib, topo):
    t = script.Topology(topo.elements, topo.resnames, topo.residue_index, mass=topo.mass, residue_seq_id=topo.residue_index + 101)
    for form, P in (('{a,b,c} = shape_weights(protein);', 1), ('{a,b,c} = shape_weights(all) in residue(4);', 1),
                    ('{a,b,c} = shape_weights(all) in resid(104:110);', 7), ('{a,b,c} = shape_weights(element(\'H\')) in resname("HOH");', 933),
                    ('s = resname("ALA")[2:8]; {a,b,c} = shape_weights(s); {e,f,g} = shape_weights(all) in s;', None)):
        ir_c = script.compile_script_native(form, t, lib=host_lib, shape=True)
        ir_py, info = script.compile_script(form, t, lib=host_lib, shape=True)
        assert ir_c.property_names() == ir_py.property_names() and ir_c.fingerprint() == ir_py.fingerprint(), form
        if P is not None:
            assert len(info["a"]["sets"]) == P
        else:
            assert len(info["a"]["sets"]) == 1 and info["a"]["sets"][0].size == 70 and [s.size for s in info["e"]["sets"]] == [10] * 7


# ---- VIAMD's call pattern ----------------------------------------------------------------------------------------------------------------

def test_interrupt_and_clear(emu_lib, oracle):
    coords, topo = blob_system(oracle, F=9)
    ir = script.compile_script(CALL_SCRIPT, topo, lib=emu_lib, shape=True)[0]
    one = evaluate(emu_lib, ir, coords, 30.0, topo.mass)
    cell = V.make_unitcell(30.0)
    ev = V.ScriptEval(coords.shape[0], ir)
    sysm, traj = V.MolSystem(coords.shape[2], mass=topo.mass, unitcell=cell), V.HostTrajectory(coords, cell)
    ev.interrupt()
    ev.frame_range(sysm, traj, 0, coords.shape[0])
    ev.clear_data()
    assert not ev.frame_mask().any() and not rows(ev, "l").any()
    assert ev.frame_range(sysm, traj, 0, coords.shape[0])
    for name in CALL_NAMES:
        assert bits_equal(rows(ev, name), rows(one, name))


MERGE_SCRIPT = '{l,p,i} = shape_weights(all); {lr,pr,ir} = shape_weights(all) in resname("ALA"); d = distance(10, 30);'


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
    ir = script.compile_script(MERGE_SCRIPT, topo, lib=lib, shape=True)[0]
    F = coords.shape[0]
    ev = V.ScriptEval(F, ir)
    beg, end = shard_frames(F, rank, world)
    cell = V.make_unitcell(30.0)
    assert ev.frame_range(V.MolSystem(coords.shape[2], mass=topo.mass, unitcell=cell), V.HostTrajectory(coords, cell), beg, end)
    reduce_eval(ev)
    assert ev.frame_mask().all()
    out = {n: ev.property_data(n).values for n in ("l", "p", "i", "lr", "pr", "ir", "d")}
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), mean=ev.property_data("pr").aggregate["mean"], **out)
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_multi_rank_merge(emu_lib, oracle, tmp_path, world):
    import torch.multiprocessing as mp
    port = 35500 + (os.getpid() % 2000) + 7 * world
    mp.spawn(_merge_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    coords, topo = blob_system(oracle, F=7)
    ir = script.compile_script(MERGE_SCRIPT, topo, lib=emu_lib, shape=True)[0]
    one = evaluate(emu_lib, ir, coords, 30.0, topo.mass)
    for r in range(world):
        z = np.load(tmp_path / f"rank{r}.npz")
        for n in ("l", "p", "i", "lr", "pr", "ir", "d"):
            assert bits_equal(z[n].reshape(7, -1), rows(one, n)), n
        assert bits_equal(z["mean"], one.property_data("pr").aggregate["mean"])


def test_export_table(emu_lib, oracle, tmp_path):
    coords, topo = blob_system(oracle, F=5)
    ir = script.compile_script('{lin,plan,iso} = shape_weights(resname("ALA"));', topo, lib=emu_lib, shape=True)[0]
    ev = evaluate(emu_lib, ir, coords, 30.0, topo.mass)
    for name in NAMES:
        y = rows(ev, name)[:, 0]
        for ext in ("xvg", "csv"):
            path = tmp_path / f"{name}.{ext}"
            ev.export_table(path, name, ext)
            text = open(path, encoding="utf-8").read()
            assert name in text, text[:400]
            nums = [ln.replace(",", " ").split() for ln in text.splitlines() if ln.strip() and ln.strip()[0] in "0123456789"]
            assert len(nums) == 5
            np.testing.assert_allclose(np.array([float(ln[1]) for ln in nums], np.float32), y, rtol=1e-5, atol=2e-6)   # six decimals in the file


# ---- VIAMD's default script through the shim, both opt-ins ---------------------------------------------------------------------------

def build_shim_shape():
    """tests/native/shim_default_script_shape.cpp linked against the product library"""
    return native_host.build_shim("shim_default_script_shape")


def test_shim_default_script_with_both_opt_ins_on_the_emulator(emu_lib, tmp_path):
    import conftest
    exe = native_host.build_shim("shim_default_script_shape", conftest.build_emu(), tmp_path / "shim_shape_emu")
    native_host.run_ok([exe, "8"], "OK frames=8 properties=7 a1=gpu lin=gpu")
