"""Backbone phi / psi and the Ramachandran density on the emulator build and in the host-only entry points: known answers,
the size edges against tests/rama_ref.py, the pin to dihedral(), the map, the filtered map, VIAMD's call patterns, the default script next
to a ramachandran statement, IR validation, the multi-rank merge and the backbone read off a topology.  tests/test_rama_gpu.py runs the
same bodies on the device."""
import os
import sys

import numpy as np
import pytest

import viamd_amd as V
from viamd_amd import _lib as L
from viamd_amd import script

import rama_cases as RC
import rama_ref as R
import test_geometry as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bb", "rama")
PI32 = np.float32(np.pi)
HALF32 = np.float32(np.pi / 2)


class Option:
    """vmd_set_option for the length of a with block"""

    def __init__(self, lib, key, value):
        self.lib, self.key, self.value = lib, key.encode(), value

    def __enter__(self):
        self.old = self.lib.vmd_set_option(self.key, self.value)

    def __exit__(self, *exc):
        self.lib.vmd_set_option(self.key, self.old)


def rama_ir(lib, n, ca, c, offsets, cls=None, names=NAMES):
    ir = V.ScriptIR(lib)
    ir.add_ramachandran(names, n, ca, c, offsets, cls)
    return ir


def table(ev, name=NAMES[0]):
    pd = ev.property_data(name)
    return pd.values.reshape(pd.dim[0], -1, 2).copy()


def counts(ev, name=NAMES[1]):
    return ev.property_data(name).map_counts.copy()


def check_map(ev, cls, link, rows=None, skip_ends=False):
    """the map property against the restatement's binning of the eval's OWN table; the float view; the sums"""
    want, sums = R.bin(table(ev), cls, link, rows=rows, skip_ends=skip_ends)
    got = counts(ev)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    pd = ev.property_data(NAMES[1])
    assert pd.is_map and pd.dim == (1, 4, 512, 512) and pd.unit_str == ("rad", "")
    assert np.array_equal(pd.map_values, want.astype(np.float32)) and pd.max_value == float(want.max())
    assert np.array_equal(want.sum(axis=(0, 1)), sums)
    return want, sums


# ---- 1. known answers ----------------------------------------------------------------------------------------------------------------

GRID = np.float32(3.0625)     # every coordinate lies on a 2^-4 grid


def _hand_chain(lib, core, offsets=None, cls=None, device=False, skip_ends=False):
    """three residues; `core` = C[0], N[1], CA[1], C[1], N[2], the five atoms of the middle segment's angles"""
    pts = np.zeros((12, 3), np.float32)
    pts[0], pts[1] = (5, 7, -3), (4, 6, -1)                   # N0, CA0
    pts[2], pts[4], pts[5], pts[6], pts[8] = core
    pts[9], pts[10] = (-3, 5, 4), (-4, 3, 6)                  # CA2, C2
    pts[3], pts[7], pts[11] = (9, 9, 9), (9, 8, 9), (9, 7, 9)     # the carbonyl O: not read
    coords = (pts + GRID).T.copy()[None]
    n, ca, c = np.array([0, 4, 8], np.int32), np.array([1, 5, 9], np.int32), np.array([2, 6, 10], np.int32)
    offsets = offsets or [0, 3]
    with Option(lib, "spec_rama_skip_ends", 1 if skip_ends else 0):
        ev = TG.evaluate(lib, rama_ir(lib, n, ca, c, offsets, cls), coords, 50.0, device=device)
    return ev, coords, (n, ca, c)


def known_answers(lib, device=False):
    ir = rama_ir(lib, [0], [1], [2], [0, 1])
    assert ir.property_names() == list(NAMES)
    assert ir.property_flags("bb") == L.FLAG_TEMPORAL and ir.property_flags("rama") == L.FLAG_MAP == 8
    # a planar all-trans chain: phi = psi = fl32(pi) exactly; every inner sample in bin (0, 0) of its class; the ends at column / row 256
    nseg = 6
    zig = np.array([(i, i % 2, 0) for i in range(3 * nseg)], np.float32) + GRID
    coords = zig.T.copy()[None]
    r = np.arange(nseg, dtype=np.int32)
    cls = np.array([0, 1, 2, 3, 0, 255], np.uint8)
    for skip in (False, True):
        with Option(lib, "spec_rama_skip_ends", int(skip)):
            ev = TG.evaluate(lib, rama_ir(lib, 3 * r, 3 * r + 1, 3 * r + 2, [0, nseg], cls), coords, 50.0, device=device)
        t = table(ev)[0]
        assert t.dtype == np.float32 and TG.bits_equal(t[1:-1], np.full((nseg - 2, 2), PI32))
        assert TG.bits_equal(t[0], [0.0, PI32]) and TG.bits_equal(t[-1], [PI32, 0.0])
        m = counts(ev)
        assert [int(m[0, 0, k]) for k in range(4)] == [1, 1, 1, 1]             # segments 1 .. 4: general, glycine, proline, pre-proline
        assert int(m[0, 256, 0]) == (0 if skip else 1)                          # segment 0: phi = +0 -> column 256, psi = pi -> row 0
        assert int(m.sum()) == (4 if skip else 5)                               # segment 5 (row 256, column 0) has class 255: never binned
        assert ev.property_data("bb").unit_str == ("", "rad") and ev.property_data("bb").aggregate is None
    # right angles: phi = +pi/2 -> column 384, psi = -pi/2 -> row 128
    ev, _, _ = _hand_chain(lib, [(1, 0, 0), (0, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1)], device=device)
    assert TG.bits_equal(table(ev)[0, 1], [HALF32, -HALF32]) and int(counts(ev)[128, 384, 0]) == 1
    # a planar cis residue: (+0, +0), absent from the map (the reference's rule); its neighbours are there
    ev, _, _ = _hand_chain(lib, [(1, 0, 0), (0, 0, 0), (0, 0, 1), (1, 0, 1), (1, 0, -1)], device=device)
    assert TG.bits_equal(table(ev)[0, 1], [0.0, 0.0]) and int(counts(ev).sum()) == 2
    # a one-segment range has no angle at all and is dropped by the same rule; it cuts the chain for its neighbours
    ev, _, _ = _hand_chain(lib, [(1, 0, 0), (0, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1)], offsets=[0, 1, 2, 3], device=device)
    assert TG.bits_equal(table(ev)[0], np.zeros((3, 2))) and int(counts(ev).sum()) == 0
    # chain ends sit at column / row 256 and are absent under spec_rama_skip_ends
    for skip in (False, True):
        ev, _, _ = _hand_chain(lib, [(1, 0, 0), (0, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1)], device=device, skip_ends=skip)
        m, t = counts(ev), table(ev)[0]
        assert t[0, 0] == 0 and t[2, 1] == 0 and t[0, 1] != 0 and t[2, 0] != 0
        assert int(m[:, 256].sum()) == (0 if skip else 1) and int(m[256, :].sum()) == (0 if skip else 1) and int(m.sum()) == (1 if skip else 3)
    # a collinear triple C[0], N[1], CA[1]: phi = +0 with the sign bit clear (D-ANGLE-DEGENERATE), psi is computed
    ev, _, _ = _hand_chain(lib, [(0, 0, -2), (0, 0, 0), (0, 0, 1), (0, 1, 1), (-1, 1, 1)], device=device)
    t = table(ev)[0, 1]
    assert t[0] == 0 and not np.signbit(t[0]) and TG.bits_equal(t[1:], [HALF32])


def test_known_answers_on_the_emulator(emu_lib):
    known_answers(emu_lib)


# ---- 2. size edges ---------------------------------------------------------------------------------------------------------------------

NSEG = (1, 2, 3, 63, 64, 65, 130)
# (box, tilt, flags): orthorhombic, triclinic (tilt 12, -8, 10 on 50 A), only x and y periodic
CELLS = [((24.0, 22.0, 20.0), (0.0, 0.0, 0.0), 7), ((50.0, 50.0, 50.0), (12.0, -8.0, 10.0), 7), ((24.0, 22.0, 20.0), (0.0, 0.0, 0.0), 3)]
F_SWEEP = 7


def size_edges(lib, box, tilt, flags, exact=True, device=False):
    """every nseg x range layout in one cell: the table against the restatement, bit-identical across batch_frames unset / 1 / 3 and across
    host-staged / resident trajectories; the map against the restatement's binning of the table"""
    bx = tuple(box) + tuple(tilt)
    for nseg in NSEG:
        coords, n, ca, c = RC.chains(100 + nseg, nseg, F_SWEEP, box, tilt, flags)
        cls = RC.mixed_classes(nseg)
        for offsets in RC.splits(nseg):
            what = f"nseg {nseg}, ranges {len(offsets) - 1}, tilt {tilt}, flags {flags}"
            ir = rama_ir(lib, n, ca, c, offsets, cls)
            got = []
            for batch in (0, 1, 3):
                with Option(lib, "batch_frames", batch):
                    ev = TG.evaluate(lib, ir, coords, box, tilt=tilt, flags=flags, device=device)
                got.append(table(ev))
                assert TG.bits_equal(got[-1], got[0]), f"{what}: batch_frames {batch}"
            if device:
                assert TG.bits_equal(table(TG.evaluate(lib, ir, coords, box, tilt=tilt, flags=flags)), got[0]), f"{what}: resident / host-staged"
            assert got[0].shape == (F_SWEEP, nseg, 2)
            TG.check_values(got[0], R.angles(coords, bx, n, ca, c, offsets, flags=flags), what, exact=exact)
            check_map(ev, cls, R.links(nseg, offsets))


@pytest.mark.parametrize("box,tilt,flags", CELLS)
def test_size_edges_on_the_emulator(emu_lib, box, tilt, flags):
    size_edges(emu_lib, box, tilt, flags)


# ---- 3. the pin to dihedral() ----------------------------------------------------------------------------------------------------------

def dihedral_pin(lib, device=False):
    """phi and psi of every inner segment are the bits of dihedral() over the same four atoms, evaluated in the same IR under
    spec_angle_radians - and stay radians without it"""
    nseg, offsets = 65, [0, 1, 3, 4, 65]
    box, tilt = (50.0, 50.0, 50.0), (12.0, -8.0, 10.0)
    coords, n, ca, c = RC.chains(7, nseg, 5, box, tilt)
    link = R.links(nseg, offsets)
    sp, sn = np.flatnonzero(link & 1), np.flatnonzero(link & 2)
    one = lambda v: [[int(i)] for i in v]
    ir = rama_ir(lib, n, ca, c, offsets)
    ir.add_dihedral_population("phi", one(c[sp - 1]), one(n[sp]), one(ca[sp]), one(c[sp]))
    ir.add_dihedral_population("psi", one(n[sn]), one(ca[sn]), one(c[sn]), one(n[sn + 1]))
    mass = np.random.default_rng(1).uniform(1, 16, coords.shape[2]).astype(np.float32)
    with Option(lib, "spec_angle_radians", 1):
        ev = TG.evaluate(lib, ir, coords, box, mass, tilt=tilt, device=device)
    t = table(ev)
    assert sp.size == 61 and sn.size == 61
    assert TG.bits_equal(t[:, sp, 0], TG.rows(ev, "phi")) and TG.bits_equal(t[:, sn, 1], TG.rows(ev, "psi"))
    assert not t[:, np.flatnonzero(~(link & 1).astype(bool)), 0].any() and not t[:, np.flatnonzero(~(link & 2).astype(bool)), 1].any()
    assert TG.bits_equal(table(TG.evaluate(lib, ir, coords, box, mass, tilt=tilt, device=device)), t)      # degrees elsewhere, radians here


def test_pin_to_dihedral_on_the_emulator(emu_lib):
    dihedral_pin(emu_lib)


# ---- 4. / 5. the map and the filtered map ------------------------------------------------------------------------------------------------

def mixed_case(nseg=65, frames=7, seed=11):
    box = (24.0, 22.0, 20.0)
    coords, n, ca, c = RC.chains(seed, nseg, frames, box)
    offsets = [0, 1, 3, 4, nseg] if nseg > 4 else [0, nseg]
    return box, coords, (n, ca, c), offsets, RC.mixed_classes(nseg), R.links(nseg, offsets)


def map_checks(lib, device=False):
    box, coords, (n, ca, c), offsets, cls, link = mixed_case()
    for skip in (False, True):
        with Option(lib, "spec_rama_skip_ends", int(skip)):
            ev = TG.evaluate(lib, rama_ir(lib, n, ca, c, offsets, cls), coords, box, device=device)
        want, sums = check_map(ev, cls, link, skip_ends=skip)
        assert (sums[1:] > 0).all() and sums[0] > 0                      # glycine, proline and pre-proline channels are populated
        dv, ds = ev.rama_density("rama", 0, coords.shape[0])
        assert np.array_equal(ds, sums) and np.array_equal(dv, want.astype(np.float32))
    # class-255 segments add nothing: the same chain with every class set to none
    ev = TG.evaluate(lib, rama_ir(lib, n, ca, c, offsets, np.full(n.size, 255, np.uint8)), coords, box, device=device)
    assert not counts(ev).any() and table(ev).any()


def test_map_on_the_emulator(emu_lib):
    map_checks(emu_lib)


def filtered_map(lib, device=False):
    box, coords, (n, ca, c), offsets, cls, link = mixed_case()
    F, N = coords.shape[0], coords.shape[2]
    ir = rama_ir(lib, n, ca, c, offsets, cls)
    ir.add_distance("d", [0], [5])
    ev = TG.evaluate(lib, ir, coords, box, device=device)
    t = table(ev)
    before = (counts(ev), t.copy(), ev.property_data("rama").fingerprint, ev.property_data("bb").fingerprint, ev.frame_mask().copy(),
              ev.property_data("rama").values.copy())
    for beg, end, rows in ((2, 5, [2, 3, 4]), (0, F, range(F)), (3, 3, []), (5, 2, []), (F, F, [])):
        want, sums = R.bin(t, cls, link, rows=rows)
        dv, ds = ev.rama_density("rama", beg, end)
        assert dv.shape == (512, 512, 4) and np.array_equal(dv, want.astype(np.float32)) and np.array_equal(ds, sums), (beg, end)
    assert np.array_equal(ev.rama_density("rama", 0, F)[0], ev.property_data("rama").map_values)
    # accumulated results and fingerprints are unchanged by the calls
    assert np.array_equal(counts(ev), before[0]) and TG.bits_equal(table(ev), before[1]) and np.array_equal(ev.frame_mask(), before[4])
    assert ev.property_data("rama").fingerprint == before[2] and ev.property_data("bb").fingerprint == before[3]
    assert np.array_equal(ev.property_data("rama").values, before[5])
    for args, msg in (((0, F + 1), "outside"), ((F - 1, F + 3), "outside")):
        with pytest.raises(V.VmdError, match=msg):
            ev.rama_density("rama", *args)
    for name, msg in (("bb", "not a ramachandran map"), ("d", "not a ramachandran map"), ("nope", "unknown property")):
        with pytest.raises(V.VmdError, match=msg):
            ev.rama_density(name, 0, F)
    # only frames 0 - 3 evaluated: the whole range answers for rows 0 - 3
    ev2 = TG.evaluate(lib, ir, coords, box, ranges=[(0, 4)], device=device)
    want, sums = R.bin(table(ev2), cls, link, rows=range(4))
    dv, ds = ev2.rama_density("rama", 0, F)
    assert sums.sum() > 0 and np.array_equal(dv, want.astype(np.float32)) and np.array_equal(ds, sums)
    assert not table(ev2)[4:].any() and np.array_equal(counts(ev2), want)
    # a query before anything was evaluated: zeros
    ev3 = V.ScriptEval(F, ir)
    dv, ds = ev3.rama_density("rama", 0, F)
    assert not dv.any() and not ds.any()


def test_filtered_map_on_the_emulator(emu_lib):
    filtered_map(emu_lib)


# ---- 6. call patterns ------------------------------------------------------------------------------------------------------------------

def call_patterns(lib, device=False):
    box, coords, (n, ca, c), offsets, cls, link = mixed_case()
    F = coords.shape[0]
    ir = rama_ir(lib, n, ca, c, offsets, cls)
    one = TG.evaluate(lib, ir, coords, box, device=device)
    want = (table(one), counts(one), one.rama_density("rama", 0, F)[1])
    assert want[1].sum() > 0
    for kw in (dict(ranges=[(f, f + 1) for f in range(F)]), dict(ranges=[(0, 3), (3, 6), (6, 7)]), dict(pooled=(4, 2))):
        ev = TG.evaluate(lib, ir, coords, box, device=device, **kw)
        assert TG.bits_equal(table(ev), want[0]) and np.array_equal(counts(ev), want[1]), kw
        dv, ds = ev.rama_density("rama", 0, F)
        assert np.array_equal(ds, want[2]) and np.array_equal(dv, want[1].astype(np.float32)), kw
        assert np.array_equal(ev.rama_density("rama", 2, 5)[0], R.bin(want[0], cls, link, rows=[2, 3, 4])[0].astype(np.float32)), kw
    # clear_data followed by a second evaluation gives the same result
    cell = V.make_unitcell(box)
    import cases
    sysm, traj = V.MolSystem(coords.shape[2], unitcell=cell), cases.make_traj(lib, coords, cell, device)
    one.clear_data()
    assert not table(one).any() and not one.property_data("rama").values.any() and not one.rama_density("rama", 0, F)[1].any()
    assert one.frame_range(sysm, traj, 0, F)
    assert TG.bits_equal(table(one), want[0]) and np.array_equal(counts(one), want[1])
    assert np.array_equal(one.rama_density("rama", 0, F)[1], want[2])


def test_call_patterns_on_the_emulator(emu_lib):
    call_patterns(emu_lib)


# ---- 7. nothing else moves ---------------------------------------------------------------------------------------------------------------

OPT_INS = dict(angles=True, shape=True, rmsd=True, within=True, shell_rdf=True, shell_sdf=True, shell_expr=True)


def nothing_else_moves(lib, oracle, device=False):
    """VIAMD's default script, compiled with the existing opt-ins, with and without a ramachandran statement in the same IR: every other
    property's values, counts and fingerprints are bit-identical"""
    atoms, blob, box, F = 6001, 200, 30.0, 20
    coords, topo = TG.blob_system(oracle, n_atoms=atoms, n_blob=blob, box=box, F=F, seed=5)
    names = np.array(["N", "CA", "C", "O", "CB", "H", "HA", "HB1", "CG", "HG"])
    topo.names = np.where(np.arange(atoms) < blob, names[np.arange(atoms) % 10], topo.elements)
    bb = script.backbone_from_topology(topo)
    assert bb["n"].size == blob // 10 and list(bb["range_offsets"]) == [0, blob // 10]
    evs = []
    for with_rama in (False, True):
        ir = script.compile_script_native(TG.VIAMD_DEFAULT_SCRIPT, topo, lib=lib, **OPT_INS)
        if with_rama:
            ir.add_ramachandran(NAMES, **bb)
        evs.append(TG.evaluate(lib, ir, coords, box, topo.mass, device=device))
    plain, both = evs
    props = plain.ir.property_names()
    assert props == ["d1", "a1", "r", "v", "lin", "plan", "iso"] and both.ir.property_names() == props + list(NAMES)
    for name in props:
        a, b = plain.property_data(name), both.property_data(name)
        assert a.dim == b.dim and a.fingerprint == b.fingerprint, name
        assert np.array_equal(a.values.view(np.int32), b.values.view(np.int32)), name
        if a.c.counts:
            assert np.array_equal(a.counts, b.counts), name
    assert counts(both).sum() > 0


def test_nothing_else_moves_on_the_emulator(emu_lib, oracle):
    nothing_else_moves(emu_lib, oracle)


# ---- 8. IR validation and fingerprint ------------------------------------------------------------------------------------------------------

def _bb(n=(0, 4, 8), ca=(1, 5, 9), c=(2, 6, 10), offsets=(0, 3), cls=None):
    return dict(n=n, ca=ca, c=c, range_offsets=offsets, rama_class=cls)


BAD = [(_bb(n=(), ca=(), c=(), offsets=(0,)), "no segment"),
       (_bb(ca=(1, -5, 9)), "negative atom index"),
       (_bb(offsets=(1, 3)), "start at 0"),
       (_bb(offsets=(0, 2, 2, 3)), "must increase"),
       (_bb(offsets=(0, 2)), "end at"),
       (_bb(cls=(0, 4, 255)), "class 4")]


@pytest.mark.parametrize("args,msg", BAD)
def test_ir_validation_errors(host_lib, args, msg):
    ir = V.ScriptIR(host_lib)
    with pytest.raises(V.VmdError, match=msg):
        ir.add_ramachandran(NAMES, **args)
    assert ir.property_count() == 0


def test_ir_validation_of_names_and_null(host_lib):
    import ctypes as C
    ir = V.ScriptIR(host_lib)
    ir.add_distance("d", [0], [1])
    for names, msg in ((("d", "m"), "already defined"), (("t", "d"), "already defined"), (("t", "t"), "already defined"), (("", "m"), "empty")):
        with pytest.raises(V.VmdError, match=msg):
            ir.add_ramachandran(names, **_bb())
    two = (C.c_char_p * 2)(b"t", b"m")
    idx = (C.c_int32 * 3)(0, 1, 2)
    off = (C.c_uint32 * 2)(0, 3)
    good = L.BackboneC(3, idx, idx, idx, 1, off, None)
    assert not host_lib.vmd_ir_add_ramachandran(ir.h, two, None) and "backbone" in host_lib.last_error()
    assert not host_lib.vmd_ir_add_ramachandran(ir.h, None, C.byref(good))
    assert not host_lib.vmd_ir_add_ramachandran(None, two, C.byref(good))
    for field in ("n", "ca", "c", "range_offsets"):
        bad = L.BackboneC(3, idx, idx, idx, 1, off, None)
        setattr(bad, field, None)
        assert not host_lib.vmd_ir_add_ramachandran(ir.h, two, C.byref(bad)), field
    assert ir.property_count() == 1
    assert host_lib.vmd_ir_add_ramachandran(ir.h, two, C.byref(good)) and ir.property_names() == ["d", "t", "m"]


def test_fingerprint_work_and_atoms(host_lib):
    def fp(**kw):
        ir = V.ScriptIR(host_lib)
        ir.add_ramachandran(NAMES, **_bb(**kw))
        return ir.fingerprint()
    base = fp()
    assert base == fp() and base == fp(cls=(0, 0, 0))                 # NULL classes are all general
    assert base != fp(n=(0, 4, 7)) and base != fp(ca=(1, 5, 11)) and base != fp(c=(3, 6, 10))
    assert base != fp(offsets=(0, 1, 3)) and base != fp(offsets=(0, 2, 3)) and fp(offsets=(0, 1, 3)) != fp(offsets=(0, 2, 3))
    assert base != fp(cls=(0, 0, 1)) and fp(cls=(0, 0, 1)) != fp(cls=(0, 0, 255))
    ir = V.ScriptIR(host_lib)
    ir.add_distance("d", [0, 1], [2, 3, 4])
    w0 = int(host_lib.vmd_ir_work_per_frame(ir.h))
    ir.add_ramachandran(NAMES, **_bb())
    assert int(host_lib.vmd_ir_work_per_frame(ir.h)) == w0 + 9
    assert list(ir.geometry_atoms("bb")) == [0, 1, 2, 4, 5, 6, 8, 9, 10] and list(ir.geometry_atoms("bb", 1)) == [4, 5, 6]
    assert ir.geometry_atoms("bb", 3).size == 0 and ir.geometry_atoms("rama").size == 0


def test_exporters(emu_lib, tmp_path):
    box, coords, (n, ca, c), offsets, cls, link = mixed_case(nseg=3, frames=2)
    ev = TG.evaluate(emu_lib, rama_ir(emu_lib, n, ca, c, offsets, cls), coords, box)
    path = tmp_path / "bb.csv"
    ev.export_table(path, "bb", fmt="csv")
    assert "bb[1]" in path.read_text() and "bb[6]" in path.read_text() and "bb[7]" not in path.read_text()
    with pytest.raises(V.VmdError, match="Ramachandran map"):
        ev.export_table(tmp_path / "m.csv", "rama", fmt="csv")
    cell = V.make_unitcell(box)
    with pytest.raises(V.VmdError, match="Ramachandran map"):
        ev.export_cube(tmp_path / "m.cube", "rama", V.MolSystem(coords.shape[2], unitcell=cell), V.HostTrajectory(coords, cell))


# ---- 9. merge ------------------------------------------------------------------------------------------------------------------------------

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
    box, coords, (n, ca, c), offsets, cls, link = mixed_case(frames=8)
    F = coords.shape[0]
    ev = V.ScriptEval(F, rama_ir(lib, n, ca, c, offsets, cls))
    beg, end = shard_frames(F, rank, world)
    cell = V.make_unitcell(box)
    assert ev.frame_range(V.MolSystem(coords.shape[2], unitcell=cell), V.HostTrajectory(coords, cell), beg, end)
    own = ev.rama_density("rama", 0, F)[1]
    reduce_eval(ev)
    assert ev.frame_mask().all()
    dv, ds = ev.rama_density("rama", 0, F)
    part = ev.rama_density("rama", 3, 6)[0]
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), t=table(ev), m=counts(ev), v=ev.property_data("rama").values, dv=dv, ds=ds, own=own,
             part=part)
    dist.destroy_process_group()


def test_two_rank_merge(emu_lib, tmp_path):
    """two evals over halves of 8 frames, merged through the host collective, equal one eval over all frames; the filtered map works on
    both afterwards, for the whole trajectory"""
    import torch.multiprocessing as mp
    port = 47500 + (os.getpid() % 2000)
    mp.spawn(_merge_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    box, coords, (n, ca, c), offsets, cls, link = mixed_case(frames=8)
    one = TG.evaluate(emu_lib, rama_ir(emu_lib, n, ca, c, offsets, cls), coords, box)
    dv, ds = one.rama_density("rama", 0, 8)
    own = np.zeros(4, np.uint64)
    for r in range(2):
        z = np.load(tmp_path / f"rank{r}.npz")
        assert TG.bits_equal(z["t"], table(one)) and np.array_equal(z["m"], counts(one))
        assert np.array_equal(z["v"], one.property_data("rama").values)
        assert np.array_equal(z["dv"], dv) and np.array_equal(z["ds"], ds)
        assert np.array_equal(z["part"], one.rama_density("rama", 3, 6)[0])
        own += z["own"]
    assert np.array_equal(own, ds) and ds.sum() > 0


# ---- 10. the backbone of a topology --------------------------------------------------------------------------------------------------------

def hand_topology():
    """ALA GLY PRO ALA | HOH HOH | ALA (no CA) | ALA PRO"""
    res = [("ALA", ["N", "CA", "C", "O", "CB"]), ("GLY", ["N", "CA", "C", "O"]), ("PRO", ["CD", "N", "CA", "C", "O"]),
           ("ALA", ["N", "H", "CA", "CB", "C", "O", "C"]), ("HOH", ["OW", "HW", "HW"]), ("HOH", ["OW", "HW", "HW"]),
           ("ALA", ["N", "C", "O"]), ("ala", ["N", "CA", "C"]), ("PRO", ["C", "CA", "N"])]
    names, resn, ri = [], [], []
    for r, (rn, atoms) in enumerate(res):
        names += atoms
        resn += [rn] * len(atoms)
        ri += [r] * len(atoms)
    el = [a[0] for a in names]
    return script.Topology(el, resn, ri, names=names)


def test_backbone_from_topology(host_lib):
    topo = hand_topology()
    py = script.backbone_from_topology(topo)
    assert list(py["n"]) == [0, 5, 10, 14, 30, 35] and list(py["ca"]) == [1, 6, 11, 16, 31, 34] and list(py["c"]) == [2, 7, 12, 18, 32, 33]
    assert list(py["range_offsets"]) == [0, 4, 6]
    assert list(py["rama_class"]) == [0, 1, 2, 0, 3, 2]          # ALA, GLY, PRO, ALA (its successor HOH is no segment) | ala before PRO, PRO
    cc = script.backbone_from_topology_native(topo, lib=host_lib)
    for k in py:
        assert py[k].dtype == cc[k].dtype and np.array_equal(py[k], cc[k]), k
    # pre-proline across a range break does not count; no protein at all: zero segments, one offset
    water = script.Topology(["O", "H", "H"], ["HOH"] * 3, [0, 0, 0], names=["OW", "HW", "HW"])
    for f in (script.backbone_from_topology, lambda t: script.backbone_from_topology_native(t, lib=host_lib)):
        e = f(water)
        assert e["n"].size == 0 and list(e["range_offsets"]) == [0] and e["rama_class"].size == 0
    ir = V.ScriptIR(host_lib)
    ir.add_ramachandran(NAMES, **py)
    assert ir.property_count() == 2
    import ctypes as C
    bad = L.TopologyC(2, None, None, None, (C.c_int32 * 2)(0, -1), None)
    assert not host_lib.vmd_topology_backbone(C.byref(bad)) and "negative residue index" in host_lib.last_error()
    assert not host_lib.vmd_topology_backbone(None)
