"""angle() / dihedral() (DESIGN S6b) on the emulator build and in the host-only entry points: known answers, bit parity with the
independent restatement tests/geometry_ref.py, ABI validation, the opt-in script front-end (C++ and Python twin), VIAMD's call pattern
(pool threads, interrupt / clear_data, multi-rank merges), export, and VIAMD's default script through the shim."""
import os
import sys

import numpy as np
import pytest

import native_host

import viamd_amd as V
from viamd_amd import _lib as L
from viamd_amd import script, synth

import geometry_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VIAMD_DEFAULT_SCRIPT = ("s1 = resname(\"ALA\")[2:8];\nd1 = distance(10,30);\na1 = angle(2,1,3) in resname(\"ALA\");\n"
                        "r = rdf(element('C'), element('H'), 10.0);\nv = sdf(s1, element('H'), 10.0);\n{lin,plan,iso} = shape_weights(all);")


def evaluate(lib, ir, coords, box, mass=None, tilt=(0.0, 0.0, 0.0), ranges=None, pooled=None, flags=L.PBC_ALL, device=False):
    """device=True: the frames are a resident DeviceTrajectory (cases.make_traj); flags: the cell's periodic-axis bits"""
    import cases
    F, _, N = coords.shape
    cell = V.make_unitcell(box, flags, tilt)
    ev = V.ScriptEval(F, ir)
    sysm = V.MolSystem(N, mass=mass, unitcell=cell)
    traj = cases.make_traj(lib, coords, cell, device)
    for beg, end in (ranges or [(0, F)]):
        assert (ev.frame_range_pooled(sysm, traj, beg, end, *pooled) if pooled else ev.frame_range(sysm, traj, beg, end))
    return ev


def rows(ev, name):
    pd = ev.property_data(name)
    return pd.values.reshape(pd.dim[0], -1).copy()


def bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def ulps(a, b):
    """distance in fp32 units in the last place; the bit patterns are mapped to one ordered line, so values on either side of 0 count
    too (+0 and -0 are 0 apart: the sign bit is checked where it matters)"""
    def line(v):
        i = np.asarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(line(a) - line(b))


def check_values(got, ref, what, exact=True):
    """exact (the emulator): bit-identical to the restatement.  Otherwise (the device, whose atan2 is ocml's) the rule of
    test_geometry_gpu._check: every value within 1 fp32 ulp, at most max(1, size // 1000) values not bit-identical."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if exact:
        assert bits_equal(got, ref), what
        return
    u = ulps(got, ref)
    off = int((got.view(np.int32) != ref.view(np.int32)).sum())
    print(f"{what}: {got.size} values, {off} not bit-identical, max {int(u.max())} ulp")
    assert u.max() <= 1, f"{what}: {int(u.max())} ulp from the reference"
    assert off <= max(1, got.size // 1000), f"{what}: {off} values not bit-identical"


def blob_system(oracle, n_atoms=1200, n_blob=200, box=30.0, F=4, seed=5):
    import cases
    coords = cases.host_frames(oracle, seed, n_atoms, box, F, n_blob=n_blob)
    topo = synth.water_box_topology(n_atoms, n_blob=n_blob)
    topo.residue_seq_id = topo.residue_index + 101            # the file's numbering: resid() selects by it
    return coords, topo


# ---- known answers -----------------------------------------------------------------------------------------------------------------

def _one_frame(lib, pts, box=50.0, tilt=(0.0, 0.0, 0.0), kind="angle"):
    xyz = np.asarray(pts, np.float32).T.copy()[None]
    ir = V.ScriptIR(lib)
    n = xyz.shape[2]
    (ir.add_angle if kind == "angle" else ir.add_dihedral)("g", *[[i] for i in range(n)])
    return float(rows(evaluate(lib, ir, xyz, box, tilt=tilt), "g")[0, 0])


def known_answers(lib):
    assert _one_frame(lib, [(1, 0, 0), (0, 0, 0), (0, 1, 0)]) == 90.0                # the angle sits at the middle argument
    assert _one_frame(lib, [(0, 0, 0), (1, 0, 0), (0, 1, 0)]) == np.float32(45.0)
    assert _one_frame(lib, [(-1, 0, 0), (0, 0, 0), (2, 0, 0)]) == 180.0               # straight
    assert _one_frame(lib, [(1, 1, 1), (1, 1, 1), (3, 0, 0)]) == 0.0                  # zero-length arm: atan2(0, 0) = 0, never NaN
    dih = lambda d: _one_frame(lib, [(1, 0, 0), (0, 0, 0), (0, 0, 1)] + [d], kind="dihedral")
    assert dih((1, 0, 1)) == 0.0                                                      # cis
    assert dih((-1, 0, 1)) == 180.0                                                   # trans: +180, never -180
    c60, s60 = np.cos(np.pi / 3), np.sin(np.pi / 3)
    assert abs(dih((c60, s60, 1)) - 60.0) < 1e-4                                      # IUPAC: clockwise seen along b -> c is positive
    assert abs(dih((c60, -s60, 1)) + 60.0) < 1e-4
    assert _one_frame(lib, [(1, 0, 0), (0, 0, 0), (2, 0, 0), (3, 1, 0)], kind="dihedral") == 0.0   # collinear arms: 0
    # a triangle straddling the periodic faces of a cube of 20 equals its unwrapped copy
    tri = np.array([(19.5, 0.5, 10.0), (0.5, 0.5, 10.0), (0.5, 19.0, 10.0)], np.float32)
    unwrapped = np.array([(-0.5, 0.5, 10.0), (0.5, 0.5, 10.0), (0.5, -1.0, 10.0)], np.float32)
    assert _one_frame(lib, tri, box=20.0) == _one_frame(lib, unwrapped, box=20.0) == 90.0
    ir = V.ScriptIR(lib)
    ir.add_angle("a", [0], [1], [2])
    assert ir.property_flags("a") == L.FLAG_TEMPORAL


def test_known_answers_on_the_emulator(emu_lib):
    known_answers(emu_lib)


TRICLINIC = ((24.0, 22.0, 20.0), (5.0, -3.0, 4.0))
DIH_POP = [[[6 + c] for c in range(4)], [[10 + c, 20 + c] for c in range(4)], [[30 + c] for c in range(4)],
           [[40 + c, 50 + c] for c in range(4)]]


def multi_atom_cell_case(lib, box, tilt=(0.0, 0.0, 0.0), flags=L.PBC_ALL, exact=True, device=False, what="cell"):
    """multi-atom, mass-weighted arguments of one angle and of a dihedral population in the given cell -> (angle, dihedral) of the
    restatement"""
    rng = np.random.default_rng(3)
    coords = rng.uniform(-6, 30, (3, 3, 60)).astype(np.float32)
    mass = rng.uniform(1, 16, 60).astype(np.float32)
    ir = V.ScriptIR(lib)
    ir.add_angle("a", [0, 1], [2], [3, 4, 5])
    ir.add_dihedral_population("d", *DIH_POP)
    ev = evaluate(lib, ir, coords, box, mass, tilt=tilt, flags=flags, device=device)
    bx = tuple(box) + tuple(tilt) if tuple(tilt) != (0.0, 0.0, 0.0) else box
    ref_a = G.values(coords, bx, [[0, 1], [2], [3, 4, 5]], mass, flags=flags)
    ref_d = G.values(coords, bx, DIH_POP, mass, flags=flags)
    check_values(rows(ev, "a"), ref_a, f"{what}: angle of multi-atom arguments", exact)
    check_values(rows(ev, "d"), ref_d, f"{what}: dihedral population", exact)
    return ref_a, ref_d


def triclinic_cell(lib, exact=True, device=False):
    multi_atom_cell_case(lib, *TRICLINIC, exact=exact, device=device, what="triclinic cell")


def test_triclinic_cell_matches_the_reference(emu_lib):
    triclinic_cell(emu_lib)


def partly_periodic_cell(lib, exact=True, device=False):
    """a slab: y open (flags 5).  The restatement's own numbers must differ from the fully periodic cell's, or the open axis is idle."""
    box = (24.0, 22.0, 20.0)
    slab = multi_atom_cell_case(lib, box, flags=5, exact=exact, device=device, what="slab, y open")
    full = multi_atom_cell_case(lib, box, exact=exact, device=device, what="the same cell, periodic")
    for s, f in zip(slab, full):
        assert (s != f).mean() > 0.5, "the open axis changes too few values"


def test_partly_periodic_cell_matches_the_reference(emu_lib):
    partly_periodic_cell(emu_lib)


# ---- parity with the reference ------------------------------------------------------------------------------------------------------

PARITY_SCRIPT = ('pa = angle(2,1,3) in resname("ALA");\npd = dihedral(1,2,3,4) in residue(2:15);\n'
                 'pr = angle(element(\'C\'), 1, 4) in resid(103:112);\npw = dihedral(1,2,3,1) in resname("HOH")[1:40];')


def parity(lib, oracle, geometric, exact=True, device=False):
    """single atoms, multi-atom mass-weighted arguments and script populations against the restatement, under spec_dist_geometric_com"""
    coords, topo = blob_system(oracle)
    F, _, N = coords.shape
    old = lib.vmd_set_option(b"spec_dist_geometric_com", geometric)
    try:
        rng = np.random.default_rng(11)
        ir = V.ScriptIR(lib)
        ir.add_angle("a1", [7], [3], [250])                                  # single atoms: the atoms' own coordinates
        multi = [rng.choice(N, 5, replace=False) for _ in range(4)]
        ir.add_angle("am", *multi[:3])
        ir.add_dihedral("dm", *multi)
        ir_src, info = script.compile_script(PARITY_SCRIPT, topo, lib=lib, angles=True)
        ev = evaluate(lib, ir, coords, 30.0, topo.mass, device=device)
        ev2 = evaluate(lib, ir_src, coords, 30.0, topo.mass, device=device)
        for name, sets in (("a1", [[7], [3], [250]]), ("am", multi[:3]), ("dm", multi)):
            check_values(rows(ev, name), G.values(coords, 30.0, sets, topo.mass, geometric=geometric), f"{name} geometric={geometric}", exact)
        for name in ("pa", "pd", "pr", "pw"):
            ref = G.values(coords, 30.0, info[name]["sets"], topo.mass, geometric=geometric)
            got = rows(ev2, name)
            assert got.shape[1] == len(info[name]["sets"][0]) > 1, name
            check_values(got, ref, f"{name} geometric={geometric}", exact)
        assert len(info["pa"]["sets"][0]) == 20 and len(info["pw"]["sets"][0]) == 40
    finally:
        lib.vmd_set_option(b"spec_dist_geometric_com", 0)
    # a one-atom set IS the atom: the same values from the raw coordinates, whatever the weights
    one = G.values(coords, 30.0, [[7], [3], [250]], None)
    check_values(rows(ev, "a1"), one, "a1 from the raw coordinates", exact)


@pytest.mark.parametrize("geometric", [0, 1])
def test_emulator_matches_reference_bit_for_bit(emu_lib, oracle, geometric):
    parity(emu_lib, oracle, geometric)


def radians_switch(lib, oracle, exact=True, device=False):
    coords, topo = blob_system(oracle, F=2)
    ir = script.compile_script('pa = angle(2,1,3) in resname("ALA"); pd = dihedral(1,2,3,4) in resname("ALA");', topo, lib=lib,
                               angles=True)[0]
    deg = evaluate(lib, ir, coords, 30.0, topo.mass, device=device)
    old = lib.vmd_set_option(b"spec_angle_radians", 1)
    try:
        rad = evaluate(lib, ir, coords, 30.0, topo.mass, device=device)
    finally:
        lib.vmd_set_option(b"spec_angle_radians", old)
    assert deg.property_data("pa").unit_str == ("", "°") and rad.property_data("pa").unit_str == ("", "rad")
    for name in ("pa", "pd"):
        info_sets = script.compile_script(f'x = {"angle(2,1,3)" if name == "pa" else "dihedral(1,2,3,4)"} in resname("ALA");', topo,
                                          lib=lib, angles=True)[1]["x"]["sets"]
        check_values(rows(rad, name), G.values(coords, 30.0, info_sets, topo.mass, radians=True), f"{name} in radians", exact)
        check_values(rows(deg, name), G.values(coords, 30.0, info_sets, topo.mass), f"{name} in degrees", exact)
        assert not np.array_equal(rows(rad, name), rows(deg, name))


def test_radians_switch(emu_lib, oracle):
    radians_switch(emu_lib, oracle)


# ---- values at the ends of the range -----------------------------------------------------------------------------------------------

def range_ends_system():
    """-> (coords float32 [1, 3, N], angle argument sets, dihedral argument sets, masks of the contexts meant to sit at 0 / at 180).
    Every coordinate lies in [2, 8) on the 2^-21 grid, so the fp32 copy is exact.  Angles: the arms a - b and c - b run along one
    direction, straight or folded back, and c is moved sideways by 0 - 64 ulps (2^-21 of an arm of 2 - 2.5: under 1e-3 degrees).
    Dihedrals: a and d stand on the same side of b - c (cis) or on opposite sides (trans), and d is turned about b - c by as much to
    either side.  The last contexts are degenerate on purpose: an operand of atan2 is -0 before `+ 0.0` there."""
    rng = np.random.default_rng(21)
    ulp = 2.0 ** -21
    dirs = np.array([d for d in np.ndindex(5, 5, 5)], np.float64) - 2.0                  # components -2 .. 2
    dirs = dirs[np.abs(dirs).max(axis=1) == 2]                                           # longest component 2: |d| in [2, 3.5]
    pts, ang, dih = [], [], []
    near0_a, near180_a, near0_d, near180_d = [], [], [], []

    def add(*p):
        pts.extend(p)
        return list(range(len(pts) - len(p), len(pts)))

    n_each = 96
    for c in range(n_each):
        b = 5.25 + rng.integers(0, 2 ** 19, 3) * ulp                                    # [5.25, 5.5)
        d = dirs[rng.integers(len(dirs))]                                                # |d| in [2, 3.5]
        k = 0 if c < 8 else int(rng.integers(1, 65))
        bump = np.zeros(3)
        bump[int(np.argmin(np.abs(d)))] = k * ulp * (1 if c % 4 < 2 else -1)             # sideways: along the arm's shortest component
        folded = c % 2 == 0
        a = b - d * (1.25 if c % 3 == 0 else 1.0)
        cc = b + (-d if folded else d) + bump
        ang.append(add(a, b, cc))
        (near0_a if folded else near180_a).append(len(ang) - 1)
    for c in range(n_each):
        b = 5.25 + rng.integers(0, 2 ** 19, 3) * ulp
        axis = c % 3
        b2 = np.zeros(3); b2[axis] = 1.0 if c % 2 else -1.25
        up = np.zeros(3); up[(axis + 1) % 3] = 2.0 if c % 4 < 2 else -2.25
        turn = np.zeros(3)
        k = 0 if c < 8 else int(rng.integers(1, 65))
        turn[(axis + 2) % 3] = k * ulp * (1 if c % 8 < 4 else -1)
        trans = c % 2 == 1
        a, cc = b + up, b + b2
        d = cc + (-up if trans else up) + turn
        dih.append(add(a, b, cc, d))
        (near180_d if trans else near0_d).append(len(dih) - 1)
    # degenerate on purpose.  An angle with a zero-length arm whose other arm has three negative components: u . v = -0.
    b = np.array([5.25, 5.375, 5.5])
    ang.append(add(b, b, b - np.array([2.0, 1.0, 0.5])))
    near0_a.append(len(ang) - 1)
    # A dihedral with b1 = -b2 / 2 (n1 = +0 exactly) and n2 = b2 x b3 all negative: n1 . n2 = -0 and y = +0 -> 0, not 180
    b2, b3 = np.array([2.0, -1.0, 0.5]), np.array([-2.5, 1.0, 0.5])
    assert (np.cross(b2, b3) < 0).all()
    a = b + b2 / 2
    dih.append(add(a, b, b + b2, b + b2 + b3))
    near0_d.append(len(dih) - 1)
    # Planar trans dihedrals on small integers: b1 . n2 sums three products that are each -0, so y = -0 before `+ 0.0` -> +180, not -180
    for b1, b2, b3 in (((-2, -2, 0), (1, -1, 0), (1, -2, 0)), ((-2, -2, 0), (1, 0, 0), (0, -2, 0)), ((-2, -2, 0), (-1, -2, 0), (-2, -1, 0))):
        b1, b2, b3 = (np.array(v, np.float64) for v in (b1, b2, b3))
        n2 = np.cross(b2, b3)
        assert all(v == 0.0 and np.signbit(v) for v in b1 * n2) and np.dot(np.cross(b1, b2), n2) < 0.0
        dih.append(add(b - b1, b, b + b2, b + b2 + b3))
        near180_d.append(len(dih) - 1)
    coords = np.asarray(pts, np.float64).T[None]
    assert coords.min() >= 2.0 and coords.max() < 8.0 and np.array_equal(coords, np.round(coords / ulp) * ulp)
    as_sets = lambda ctx: [[[c[k]] for c in ctx] for k in range(len(ctx[0]))]
    return coords.astype(np.float32), as_sets(ang), as_sets(dih), (near0_a, near180_a, near0_d, near180_d)


def range_ends(lib, exact=True, device=False):
    """0 <= angle <= 180 and -180 < dihedral <= 180; where the restatement gives exactly 0 or +180 so does the kernel, sign bit
    included; every value within 1 ulp of the restatement (the emulator: bit-identical).  Both sides form the operands of atan2 by the
    same uncontracted fp64 operations: only atan2 itself and the final rounding can differ."""
    coords, ang, dih, (near0_a, near180_a, near0_d, near180_d) = range_ends_system()
    ir = V.ScriptIR(lib)
    ir.add_angle_population("a", *ang)
    ir.add_dihedral_population("d", *dih)
    ev = evaluate(lib, ir, coords, 64.0, device=device)
    got_a, got_d = rows(ev, "a")[0], rows(ev, "d")[0]
    ref_a, ref_d = G.values(coords, 64.0, ang)[0], G.values(coords, 64.0, dih)[0]
    # the inputs are what they are meant to be (the restatement's own numbers)
    assert (ref_a[near0_a] < 1e-3).all() and (ref_a[near180_a] > 180.0 - 1e-3).all()
    assert (np.abs(ref_d[near0_d]) < 1e-3).all() and (np.abs(ref_d[near180_d]) > 180.0 - 1e-3).all()
    assert (ref_a == 0.0).sum() >= 4 and (ref_a == 180.0).sum() >= 4 and (ref_d == 0.0).sum() >= 4 and (ref_d == 180.0).sum() >= 4
    assert (ref_d[near180_d] < 0.0).sum() >= 20 and (ref_d[near180_d] > 0.0).sum() >= 20             # both sides of trans
    assert (ref_d[near0_d] < 0.0).sum() >= 20 and ((ref_a > 0.0) & (ref_a < 1e-3)).sum() >= 20
    for what, got, ref in (("angles at the ends of the range", got_a, ref_a), ("dihedrals at the ends of the range", got_d, ref_d)):
        assert np.isfinite(got).all(), what
        for end in (0.0, 180.0):
            at = ref == np.float32(end)
            assert np.array_equal(got[at].view(np.int32), ref[at].view(np.int32)), f"{what}: {got[at]} where the reference has +{end}"
        u = ulps(got, ref)
        print(f"{what}: {got.size} values, {int((got.view(np.int32) != ref.view(np.int32)).sum())} not bit-identical, max {int(u.max())} ulp")
        assert u.max() <= 1, f"{what}: {int(u.max())} ulp from the reference"
        assert not exact or bits_equal(got, ref), what
    assert got_a.min() >= 0.0 and got_a.max() <= 180.0 and not np.signbit(got_a[got_a == 0.0]).any()
    assert got_d.min() > -180.0 and got_d.max() <= 180.0


def test_values_at_the_ends_of_the_range_on_the_emulator(emu_lib):
    range_ends(emu_lib)


def _ala(topo):
    return [topo.residue_atoms(r) for r in range(topo.num_residues) if topo.residue_name(r) == "ALA"]


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------

def test_ir_validation_errors(host_lib):
    lib = host_lib
    ir = V.ScriptIR(lib)
    with pytest.raises(V.VmdError, match="empty"):
        ir.add_angle("e", [], [1], [2])
    with pytest.raises(V.VmdError, match="empty"):
        ir.add_dihedral("e", [0], [1], [2], [])
    with pytest.raises(V.VmdError, match="negative"):
        ir.add_angle("n", [0], [-1], [2])
    with pytest.raises(V.VmdError, match="negative"):
        ir.add_dihedral_population("n", [[0]], [[1]], [[2]], [[-3]])
    with pytest.raises(V.VmdError, match="empty"):
        ir.add_angle_population("p", [[0], []], [[1], [2]], [[3], [4]])          # offsets that do not increase
    a = np.array([0, 1], np.int32)
    off = np.array([0, 1, 1], np.int32)
    ok = np.array([0, 1, 2], np.int32)
    p = lambda x: x.ctypes.data_as(L.c_int32_p)
    assert not lib.vmd_ir_add_angle_population(ir.h, b"q", 2, p(a), p(ok), p(a), p(off), p(a), p(ok))
    assert "empty" in lib.last_error()
    bad0 = np.array([1, 2, 3], np.int32)
    assert not lib.vmd_ir_add_angle_population(ir.h, b"q", 2, p(a), p(bad0), p(a), p(ok), p(a), p(ok))
    assert "start at 0" in lib.last_error()
    assert not lib.vmd_ir_add_angle_population(ir.h, b"q", 0, p(a), p(ok), p(a), p(ok), p(a), p(ok))
    assert "empty" in lib.last_error()
    assert ir.property_count() == 0
    ir.add_angle("a", [0], [1], [2])
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_dihedral("a", [0], [1], [2], [3])
    assert not lib.vmd_ir_add_distance(ir.h, b"k4", 4, p(a), 2, p(a), 2)             # the distance kinds stay 0..3
    assert "unknown distance kind" in lib.last_error()
    # out-of-range atoms are refused when the eval meets the trajectory
    ir2 = V.ScriptIR(lib)
    ir2.add_dihedral("d", [0], [1], [2], [99])
    if lib.vmd_device_count() > 0:
        with pytest.raises(V.VmdError, match="references atom 99"):
            evaluate(lib, ir2, np.zeros((1, 3, 10), np.float32), 10.0)


def test_fingerprint_and_work(host_lib):
    def fp(build):
        ir = V.ScriptIR(host_lib)
        build(ir)
        return ir.fingerprint(), int(host_lib.vmd_ir_work_per_frame(ir.h))
    f_ang, w_ang = fp(lambda ir: ir.add_angle("x", [0, 1], [2], [3]))
    f_dih, w_dih = fp(lambda ir: ir.add_dihedral("x", [0, 1], [2], [3], [4]))
    f_dih2, _ = fp(lambda ir: ir.add_dihedral("x", [0, 1], [2], [3], [5]))
    f_dst, _ = fp(lambda ir: ir.add_distance("x", [0, 1], [2]))
    f_pop, w_pop = fp(lambda ir: ir.add_angle_population("x", [[0], [1, 2]], [[3], [4]], [[5, 6, 7], [8]]))
    assert len({f_ang, f_dih, f_dih2, f_dst, f_pop}) == 5
    assert (w_ang, w_dih, w_pop) == (4, 5, 9)
    ir = V.ScriptIR(host_lib)
    ir.add_angle_population("x", [[0], [1, 2]], [[3], [4]], [[5, 6, 7], [8]])
    assert list(ir.geometry_atoms("x")) == [0, 3, 5, 6, 7, 1, 2, 4, 8]
    assert list(ir.geometry_atoms("x", 1)) == [1, 2, 4, 8]
    ir.add_distance("d", [0], [1])
    assert ir.geometry_atoms("d").size == 0


# ---- front-end -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def topo():
    return synth.water_box_topology(200 + 933 * 3, n_blob=200)


def test_default_script_without_the_opt_in_is_unchanged(host_lib, topo):
    text = VIAMD_DEFAULT_SCRIPT
    ir_c, rep_c = script.compile_script_native(text, topo, lib=host_lib, partial=True)
    ir_e, rep_e = script.compile_script_native(text, topo, lib=host_lib, partial=True, angles=False)
    ir_py, _, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, angles=False)
    assert ir_c.property_names() == ir_e.property_names() == ir_py.property_names() == ["d1", "r", "v"]
    assert ir_c.fingerprint() == ir_e.fingerprint() == ir_py.fingerprint()
    assert rep_c == rep_e == rep_py
    assert [k["names"] for k in rep_c["skipped"]] == ["a1", "lin,plan,iso"]
    # the _ex entry point with features = 0 is the old one, strict and partial
    import ctypes as C
    n = topo.num_atoms
    strings = lambda arr: (C.c_char_p * n)(*[str(v).encode() for v in arr])
    el, rn = strings(topo.elements), strings(topo.resnames)
    ri = np.ascontiguousarray(topo.residue_index, np.int32)
    tc = L.TopologyC(n, el, el, rn, ri.ctypes.data_as(L.c_int32_p), None)
    ir_x = V.ScriptIR(host_lib)
    rep = C.c_void_p()
    assert host_lib.vmd_ir_compile_from_source_ex(ir_x.h, text.encode(), C.byref(tc), 0, C.byref(rep))
    fb = host_lib.vmd_script_report_fallback_source(rep).decode()
    assert host_lib.vmd_script_report_skipped_count(rep) == 2 and fb == rep_c["fallback_source"]
    host_lib.vmd_script_report_free(rep)
    assert ir_x.fingerprint() == ir_c.fingerprint()
    assert not host_lib.vmd_ir_compile_from_source_ex(V.ScriptIR(host_lib).h, text.encode(), C.byref(tc), 0, None)
    assert "angle" in host_lib.last_error()


def test_default_script_with_the_opt_in(host_lib, topo):
    text = VIAMD_DEFAULT_SCRIPT
    ir_c, rep_c = script.compile_script_native(text, topo, lib=host_lib, partial=True, angles=True)
    ir_py, info, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, angles=True)
    assert ir_c.property_names() == ir_py.property_names() == ["d1", "a1", "r", "v"]
    assert ir_c.fingerprint() == ir_py.fingerprint()
    assert ir_c.property_flags("a1") == L.FLAG_TEMPORAL
    assert rep_c == rep_py
    assert [k["names"] for k in rep_c["skipped"]] == ["lin,plan,iso"]
    fb = rep_c["fallback_source"]
    assert len(fb) == len(text) and "angle" not in fb and "{lin,plan,iso} = shape_weights(all);" in fb
    # a1: atoms 2, 1, 3 of each ALA residue (local, 1-based)
    ala = _ala(topo)
    assert [len(s) for s in info["a1"]["sets"]] == [20, 20, 20]
    assert [int(s[0]) for s in info["a1"]["sets"][1]] == [int(r[0]) for r in ala]
    assert list(ir_c.geometry_atoms("a1", 3)) == [int(ala[3][1]), int(ala[3][0]), int(ala[3][2])]
    # the strict form takes the script without shape_weights
    strict = text.replace("{lin,plan,iso} = shape_weights(all);", "")
    assert script.compile_script_native(strict, topo, lib=host_lib, angles=True).fingerprint() == ir_c.fingerprint()
    with pytest.raises(script.ScriptError):
        script.compile_script_native(strict, topo, lib=host_lib)


PICKING_FORMS = [
    'x = angle(12, 11, 13);',
    'x = angle(2, 1, 3) in residue(4);',
    'x = angle(2, 1, 3) in resid(104);',
    'x = angle(2, 1, 3) in resname("ALA");',
    'x = dihedral(1, 2, 3, 4);',
    'x = dihedral(1, 2, 3, 5) in residue(7);',
    'x = dihedral(1, 2, 3, 5) in resid(107);',
    'x = dihedral(1, 2, 3, 5) in resname("ALA");',
]


@pytest.mark.parametrize("form", PICKING_FORMS)
def test_picking_menu_forms(host_lib, topo, form):
    t = script.Topology(topo.elements, topo.resnames, topo.residue_index, mass=topo.mass, residue_seq_id=topo.residue_index + 101)
    ir_c = script.compile_script_native(form, t, lib=host_lib, angles=True)
    ir_py, info = script.compile_script(form, t, lib=host_lib, angles=True)
    assert ir_c.property_names() == ir_py.property_names() == ["x"]
    assert ir_c.fingerprint() == ir_py.fingerprint()
    P = len(info["x"]["sets"][0])
    assert P == (20 if "resname" in form else 1)
    nargs = 3 if "angle" in form else 4
    assert len(info["x"]["sets"]) == nargs and all(len(s) == P for s in info["x"]["sets"])
    if "residue(4)" in form or "resid(104)" in form:
        r = t.residue_atoms(3)
        assert [int(s[0][0]) for s in info["x"]["sets"]] == [int(r[1]), int(r[0]), int(r[2])]
    with pytest.raises(script.ScriptError, match="unsupported function"):
        script.compile_script_native(form, t, lib=host_lib)
    with pytest.raises(script.ScriptError, match="unsupported function"):
        script.compile_script(form, t, lib=host_lib)


# ---- call pattern ---------------------------------------------------------------------------------------------------------------------

def test_pool_threads_interrupt_and_clear(emu_lib, oracle):
    coords, topo = blob_system(oracle, F=9)
    src = 'pa = angle(2,1,3) in resname("ALA"); pd = dihedral(1,2,3,4) in resname("ALA");'
    ir = script.compile_script(src, topo, lib=emu_lib, angles=True)[0]
    one = evaluate(emu_lib, ir, coords, 30.0, topo.mass)
    pool = evaluate(emu_lib, ir, coords, 30.0, topo.mass, pooled=(16, 1))
    parts = evaluate(emu_lib, ir, coords, 30.0, topo.mass, ranges=[(0, 2), (2, 7), (7, 9)])
    for name in ("pa", "pd"):
        assert bits_equal(rows(pool, name), rows(one, name)) and bits_equal(rows(parts, name), rows(one, name))
        agg = one.property_data(name).aggregate
        r = rows(one, name)
        np.testing.assert_allclose(agg["mean"], r.mean(axis=1), rtol=1e-5, atol=1e-4)
        np.testing.assert_array_equal(agg["ext"][:, 0], r.min(axis=1))
    cell = V.make_unitcell(30.0)
    ev = V.ScriptEval(coords.shape[0], ir)
    sysm, traj = V.MolSystem(coords.shape[2], mass=topo.mass, unitcell=cell), V.HostTrajectory(coords, cell)
    ev.interrupt()
    ev.frame_range(sysm, traj, 0, coords.shape[0])
    ev.clear_data()
    assert ev.frame_range(sysm, traj, 0, coords.shape[0])
    for name in ("pa", "pd"):
        assert bits_equal(rows(ev, name), rows(one, name))


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
    ir = script.compile_script('pa = angle(2,1,3) in resname("ALA"); d = distance(10, 30);', topo, lib=lib, angles=True)[0]
    F = coords.shape[0]
    ev = V.ScriptEval(F, ir)
    beg, end = shard_frames(F, rank, world)
    cell = V.make_unitcell(30.0)
    assert ev.frame_range(V.MolSystem(coords.shape[2], mass=topo.mass, unitcell=cell), V.HostTrajectory(coords, cell), beg, end)
    reduce_eval(ev)
    assert ev.frame_mask().all()
    pd = ev.property_data("pa")
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), pa=pd.values, mean=pd.aggregate["mean"], d=ev.property_data("d").values)
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_multi_rank_merge_of_an_angle_population(emu_lib, oracle, tmp_path, world):
    import torch.multiprocessing as mp
    port = 33500 + (os.getpid() % 2000) + 7 * world
    mp.spawn(_merge_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    coords, topo = blob_system(oracle, F=7)
    ir = script.compile_script('pa = angle(2,1,3) in resname("ALA"); d = distance(10, 30);', topo, lib=emu_lib, angles=True)[0]
    one = evaluate(emu_lib, ir, coords, 30.0, topo.mass)
    for r in range(world):
        z = np.load(tmp_path / f"rank{r}.npz")
        assert bits_equal(z["pa"].reshape(7, -1), rows(one, "pa"))
        assert bits_equal(z["mean"], one.property_data("pa").aggregate["mean"])
        assert bits_equal(z["d"], one.property_data("d").values)


# ---- export ---------------------------------------------------------------------------------------------------------------------------

def test_export_labels_the_unit(emu_lib, oracle, tmp_path):
    import ctypes as C
    coords, topo = blob_system(oracle, F=3)
    ir = script.compile_script('a1 = angle(2,1,3) in resname("ALA")[1:1];', topo, lib=emu_lib, angles=True)[0]
    for radians, unit in ((0, "°"), (1, "rad")):
        old = emu_lib.vmd_set_option(b"spec_angle_radians", radians)
        try:
            ev = evaluate(emu_lib, ir, coords, 30.0, topo.mass)
        finally:
            emu_lib.vmd_set_option(b"spec_angle_radians", old)
        pd = ev.property_data("a1")
        u = pd.unit_str[1]
        assert u == unit
        y_label = f"a1 ({u})" if u else "a1"                     # VIAMD's column label: "label (unit)" when the unit is not none
        x = np.arange(3, dtype=np.float32)
        y = np.ascontiguousarray(pd.values, np.float32)
        cols = (L.c_float_p * 2)(x.ctypes.data_as(L.c_float_p), y.ctypes.data_as(L.c_float_p))
        labels = (C.c_char_p * 2)(b"Frame", y_label.encode())
        for fn, ext in ((emu_lib.vmd_export_xvg, "xvg"), (emu_lib.vmd_export_csv, "csv")):
            path = str(tmp_path / f"a1_{radians}.{ext}")
            assert fn(path.encode(), cols, labels, 2, 3)
            text = open(path, encoding="utf-8").read()
            assert f"a1 ({unit})" in text, text[:400]
            nums = [ln.replace(",", " ").split() for ln in text.splitlines() if ln.strip() and ln.strip()[0] in "0123456789"]
            assert len(nums) == 3
            got = np.array([float(ln[1]) for ln in nums], np.float32)
            np.testing.assert_allclose(got, y, rtol=1e-5, atol=2e-6)       # six decimals in the file


# ---- VIAMD's default script through the shim, angles opted in ----------------------------------------------------------------------

def build_shim_angles():
    """tests/native/shim_default_script_angles.cpp linked against the product library"""
    return native_host.build_shim("shim_default_script_angles")


def test_shim_default_script_with_angles_on_the_emulator(emu_lib, tmp_path):
    import conftest
    exe = native_host.build_shim("shim_default_script_angles", conftest.build_emu(), tmp_path / "shim_angles_emu")
    native_host.run_ok([exe, "8"], "OK frames=8 properties=7 a1=gpu")
