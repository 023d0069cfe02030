"""angle() / dihedral() (DESIGN S6b) on the emulator build and in the host-only entry points: known answers, bit parity with the
independent restatement tests/geometry_ref.py, ABI validation, the opt-in script front-end (C++ and Python twin), VIAMD's call pattern
(pool threads, interrupt / clear_data, multi-rank merges), export, and VIAMD's default script through the shim."""
import os
import subprocess
import sys

import numpy as np
import pytest

import viamd_amd as V
from viamd_amd import _lib as L
from viamd_amd import script, synth

import geometry_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_ANGLES_SRC = os.path.join(ROOT, "tests", "native", "shim_default_script_angles.cpp")
SHIM_ANGLES_EXE = os.path.join(ROOT, "tests", "native", "shim_default_script_angles")

VIAMD_DEFAULT_SCRIPT = ("s1 = resname(\"ALA\")[2:8];\nd1 = distance(10,30);\na1 = angle(2,1,3) in resname(\"ALA\");\n"
                        "r = rdf(element('C'), element('H'), 10.0);\nv = sdf(s1, element('H'), 10.0);\n{lin,plan,iso} = shape_weights(all);")


def evaluate(lib, ir, coords, box, mass=None, tilt=(0.0, 0.0, 0.0), ranges=None, pooled=None):
    F, _, N = coords.shape
    cell = V.make_unitcell(box, tilt=tilt)
    ev = V.ScriptEval(F, ir)
    sysm = V.MolSystem(N, mass=mass, unitcell=cell)
    traj = V.HostTrajectory(coords, cell)
    for beg, end in (ranges or [(0, F)]):
        assert (ev.frame_range_pooled(sysm, traj, beg, end, *pooled) if pooled else ev.frame_range(sysm, traj, beg, end))
    return ev


def rows(ev, name):
    pd = ev.property_data(name)
    return pd.values.reshape(pd.dim[0], -1).copy()


def bits_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


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


def test_known_answers_on_the_emulator(emu_lib):
    lib = emu_lib
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


def test_triclinic_cell_matches_the_reference(emu_lib):
    rng = np.random.default_rng(3)
    box, tilt = (24.0, 22.0, 20.0), (5.0, -3.0, 4.0)
    coords = rng.uniform(-6, 30, (3, 3, 60)).astype(np.float32)
    mass = rng.uniform(1, 16, 60).astype(np.float32)
    ir = V.ScriptIR(emu_lib)
    ir.add_angle("a", [0, 1], [2], [3, 4, 5])
    ir.add_dihedral_population("d", [[6 + c] for c in range(4)], [[10 + c, 20 + c] for c in range(4)], [[30 + c] for c in range(4)],
                               [[40 + c, 50 + c] for c in range(4)])
    ev = evaluate(emu_lib, ir, coords, box, mass, tilt=tilt)
    assert bits_equal(rows(ev, "a"), G.values(coords, box + tilt, [[0, 1], [2], [3, 4, 5]], mass))
    ref = G.values(coords, box + tilt, [[[6 + c] for c in range(4)], [[10 + c, 20 + c] for c in range(4)], [[30 + c] for c in range(4)],
                                        [[40 + c, 50 + c] for c in range(4)]], mass)
    assert bits_equal(rows(ev, "d"), ref)


# ---- parity with the reference ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geometric", [0, 1])
def test_emulator_matches_reference_bit_for_bit(emu_lib, oracle, geometric):
    coords, topo = blob_system(oracle)
    F, _, N = coords.shape
    old = emu_lib.vmd_set_option(b"spec_dist_geometric_com", geometric)
    try:
        rng = np.random.default_rng(11)
        ir = V.ScriptIR(emu_lib)
        ir.add_angle("a1", [7], [3], [250])                                  # single atoms: the atoms' own coordinates
        multi = [rng.choice(N, 5, replace=False) for _ in range(4)]
        ir.add_angle("am", *multi[:3])
        ir.add_dihedral("dm", *multi)
        src = ('pa = angle(2,1,3) in resname("ALA");\npd = dihedral(1,2,3,4) in residue(2:15);\n'
               'pr = angle(element(\'C\'), 1, 4) in resid(103:112);\npw = dihedral(1,2,3,1) in resname("HOH")[1:40];')
        ir_src, info = script.compile_script(src, topo, lib=emu_lib, angles=True)
        ev = evaluate(emu_lib, ir, coords, 30.0, topo.mass)
        ev2 = evaluate(emu_lib, ir_src, coords, 30.0, topo.mass)
        for name, sets in (("a1", [[7], [3], [250]]), ("am", multi[:3]), ("dm", multi)):
            assert bits_equal(rows(ev, name), G.values(coords, 30.0, sets, topo.mass, geometric=geometric)), name
        for name in ("pa", "pd", "pr", "pw"):
            ref = G.values(coords, 30.0, info[name]["sets"], topo.mass, geometric=geometric)
            got = rows(ev2, name)
            assert got.shape[1] == len(info[name]["sets"][0]) > 1 and bits_equal(got, ref), name
        assert len(info["pa"]["sets"][0]) == 20 and len(info["pw"]["sets"][0]) == 40
    finally:
        emu_lib.vmd_set_option(b"spec_dist_geometric_com", 0)
    # a one-atom set IS the atom: the same values from the raw coordinates, whatever the weights
    one = G.values(coords, 30.0, [[7], [3], [250]], None)
    assert bits_equal(rows(ev, "a1"), one)


def test_radians_switch(emu_lib, oracle):
    coords, topo = blob_system(oracle, F=2)
    ir = script.compile_script('pa = angle(2,1,3) in resname("ALA"); pd = dihedral(1,2,3,4) in resname("ALA");', topo, lib=emu_lib,
                               angles=True)[0]
    deg = evaluate(emu_lib, ir, coords, 30.0, topo.mass)
    old = emu_lib.vmd_set_option(b"spec_angle_radians", 1)
    try:
        rad = evaluate(emu_lib, ir, coords, 30.0, topo.mass)
    finally:
        emu_lib.vmd_set_option(b"spec_angle_radians", old)
    assert deg.property_data("pa").unit_str == ("", "°") and rad.property_data("pa").unit_str == ("", "rad")
    for name in ("pa", "pd"):
        info_sets = script.compile_script(f'x = {"angle(2,1,3)" if name == "pa" else "dihedral(1,2,3,4)"} in resname("ALA");', topo,
                                          lib=emu_lib, angles=True)[1]["x"]["sets"]
        assert bits_equal(rows(rad, name), G.values(coords, 30.0, info_sets, topo.mass, radians=True))
        assert bits_equal(rows(deg, name), G.values(coords, 30.0, info_sets, topo.mass))
        assert not np.array_equal(rows(rad, name), rows(deg, name))


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

def build_shim_angles(lib_path=None):
    """tests/native/shim_default_script_angles.cpp linked against the product library (or `lib_path`, e.g. the emulator build)"""
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "native")]
    if lib_path:
        out = lib_path + ".shim_angles"
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", SHIM_ANGLES_SRC] + inc + [lib_path, "-Wl,-rpath," + os.path.dirname(lib_path),
                               "-lpthread", "-o", out])
        return out
    from viamd_amd import build
    lib = build.build()
    deps = [SHIM_ANGLES_SRC, lib, os.path.join(ROOT, "include", "vmd_md_script_shim.h"), os.path.join(ROOT, "tests", "native", "md_mock.h"),
            os.path.join(ROOT, "tests", "native", "md_mock_eval.h")]
    if os.path.exists(SHIM_ANGLES_EXE) and os.path.getmtime(SHIM_ANGLES_EXE) >= max(os.path.getmtime(d) for d in deps):
        return SHIM_ANGLES_EXE
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SHIM_ANGLES_SRC] + inc + ["-L" + os.path.join(ROOT, "viamd_amd"), "-lviamd_amd",
                           "-L/opt/rocm/lib", "-Wl,-rpath,$ORIGIN/../../viamd_amd", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib",
                           "-lpthread", "-o", SHIM_ANGLES_EXE])
    return SHIM_ANGLES_EXE


def test_shim_default_script_with_angles_on_the_emulator(emu_lib, tmp_path):
    import conftest
    emu = conftest.build_emu()
    exe = str(tmp_path / "shim_angles_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", SHIM_ANGLES_SRC, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tests", "native"), emu, "-Wl,-rpath," + os.path.dirname(emu), "-lpthread", "-o", exe])
    out = subprocess.run([exe, "8"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("OK frames=8 properties=7 a1=gpu"), out.stdout
