"""Per-frame secondary structure on the emulator build and in the host-only entry points: known answers on ideal backbones,
the size edges against tests/ss_ref.py (every value, exact), the coverage the inputs must have, inputs at the two thresholds, IR
validation, the statement next to the other forms, VIAMD's call patterns and the multi-rank merge.  tests/test_ss_gpu.py runs the same
bodies on the device.  (DESIGN 1.11 sends a new form's IR cases to tests/ir_cases.py and its statement to tests/test_forms_together.py;
this form's stand here, sections 5 and 6.)"""
import os
import sys

import numpy as np
import pytest

import viamd_amd as V
from viamd_amd import _lib as L
from viamd_amd import script

import rama_cases as RC
import ss_cases as SC
import ss_ref as R
import test_geometry as TG
from test_rama import CELLS, OPT_INS, Option

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ss", "sspop")
BIG = (60.0, 60.0, 60.0)


def ss_ir(lib, n, ca, c, o, offsets, cls=None, names=NAMES):
    ir = V.ScriptIR(lib)
    ir.add_secondary_structure(names, n, ca, c, o, offsets, cls)
    return ir


def classes(ev, name=NAMES[0]):
    return ev.property_data(name).ss_classes


def pops(ev, name=NAMES[1]):
    pd = ev.property_data(name)
    return pd.values.reshape(pd.dim[0], pd.dim[1]).copy()


def explain(got, want, details, what):
    """every segment whose code differs: both codes and, from the restatement, the bonds it evaluated for that segment as a donor and as
    an acceptor - the four distances and the energy"""
    lines = []
    for f, s in zip(*np.nonzero(got != want)):
        lines.append(f"{what}: frame {f} segment {s}: got {got[f, s]} want {want[f, s]}")
        d = details[f]
        for a, dn in zip(*np.nonzero(d["evaluated"])):
            if s in (a, dn):
                r = [float(q[a, dn]) for q in d["r"]]
                lines.append(f"    hb({a}, {dn}) = {bool(d['hb'][a, dn])}: rON rCH rOH rCN = {r}, E = {float(d['energy'][a, dn])!r}, CA^2 = {float(d['gate2'][a, dn])!r}")
    return "\n".join(lines[:200])


def check(ev, want, details, what):
    got = classes(ev)
    assert got.dtype == np.uint8 and got.shape == want.shape, what
    if not np.array_equal(got, want):
        print(explain(got, want, details, what))
    assert np.array_equal(got, want), what
    assert np.array_equal(pops(ev), R.populations(want)), what


# ---- 1. known answers ----------------------------------------------------------------------------------------------------------------

# name -> (builder, range offsets, the plain answer, residue 6 a proline, o[3] = -1)
IDEAL = {
    "alpha": (lambda: SC.ideal(-57.0, -47.0, 14), [0, 14], "-HHHHHHHHHHHH-", "-HHHHHHHHHHHH-", "--HHHHHHHHHHH-"),
    "3-10": (lambda: SC.ideal(-49.0, -26.0, 14), [0, 14], "-GGGGGGGGGGGG-", "-GGGGGGGGGGGG-", "-TTTTGGGGGGGG-"),
    "pi": (lambda: SC.ideal(-57.0, -70.0, 14), [0, 14], "-IIIIIIIIIIII-", "-TTIIIIIIIIII-", "-IIIIIIIIIIII-"),
    "extended": (lambda: SC.ideal(-120.0, 130.0, 14), [0, 14], "-" * 14, "-" * 14, "-" * 14),
    "parallel": (lambda: SC.sheet(True), [0, 8, 16], "-EEEEEE--EEEEEE-", "-EEEE----EEEE---", "-EE--EE--EE--EE-"),
    "antiparallel": (lambda: SC.sheet(False), [0, 8, 16], "-EEEEEE--EEEEEE-", "-EEEE------EEEE-", "-EE--EE--EE--EE-"),
}
CUT = {"alpha": "-HHHHH--HHHHH-", "3-10": "-GGGGG--GGGGG-", "pi": "-IIIII--IIIII-"}       # the helix in two ranges of seven


def known_answers(lib, device=False):
    ir = ss_ir(lib, [0], [1], [2], [3], [0, 1])
    assert ir.property_names() == list(NAMES)
    assert ir.property_flags("ss") == L.FLAG_TEMPORAL and ir.property_flags("sspop") == L.FLAG_TEMPORAL
    for name, (build, offsets, plain, proline, no_o) in IDEAL.items():
        xyz = build()
        nseg = len(xyz) // 4
        n, ca, c, o = SC.backbone(nseg)
        coords = SC.frames_of(xyz, BIG)
        pro = np.zeros(nseg, np.uint8)
        pro[6] = 2
        o3 = o.copy()
        o3[3] = -1
        variants = [(offsets, None, o, plain), (offsets, pro, o, proline), (offsets, None, o3, no_o)]
        if name in CUT:
            variants.append(([0, 7, 14], None, o, CUT[name]))
        for off, cls, ox, answer in variants:
            det = []
            want = R.classes(coords, BIG, n, ca, c, ox, off, cls, details=det)
            assert R.letters(want[0]) == answer, (name, R.letters(want[0]))
            if cls is not None:
                assert not det[0]["donor"][6]                                          # a proline donates no H
            if ox is o3:
                assert not det[0]["hb"][3].any() and not det[0]["hb"][:, 4].any()       # 3 never accepts, 4 never donates
            ev = TG.evaluate(lib, ss_ir(lib, n, ca, c, ox, off, cls), coords, BIG, device=device)
            check(ev, want, det, name)
            assert "".join(L.SS_LETTERS[k] for k in classes(ev)[0]) == answer, name
            pd, pq = ev.property_data("ss"), ev.property_data("sspop")
            assert pd.dim[:2] == (1, nseg) and pq.dim[:2] == (1, 9) and pd.unit_str == ("", "") and pq.unit_str == ("", "")
            assert pd.aggregate is None and pq.aggregate is None
            assert pops(ev)[0].sum() == nseg and pops(ev)[0, 0] == 0
    # a frame that was not evaluated reads all 0 (VMD_SS_UNKNOWN) in both records
    xyz = SC.ideal(-57.0, -47.0, 14)
    n, ca, c, o = SC.backbone(14)
    coords = np.repeat(SC.frames_of(xyz, BIG), 3, axis=0)
    ev = TG.evaluate(lib, ss_ir(lib, n, ca, c, o, [0, 14]), coords, BIG, ranges=[(1, 2)], device=device)
    assert not classes(ev)[[0, 2]].any() and not pops(ev)[[0, 2]].any()
    assert R.letters(classes(ev)[1]) == "-HHHHHHHHHHHH-" and pops(ev)[1, R.HELIX_ALPHA] == 12


def test_known_answers_on_the_emulator(emu_lib):
    known_answers(emu_lib)


# ---- 2. size edges ---------------------------------------------------------------------------------------------------------------------

NSEG = (1, 2, 3, 5, 6, 7, 63, 64, 65, 66, 127, 128, 129, 130)
F_SWEEP = 5
_SWEEP = {}


def sweep_case(cell, nseg):
    """the planted frames of one (cell, nseg) and, per range layout, the restatement's classes and details: made once, shared, never changed"""
    key = (cell, nseg)
    if key not in _SWEEP:
        box, tilt, flags = CELLS[cell]
        coords, (n, ca, c, o), _ = SC.planted(1000 + nseg + cell, nseg, F_SWEEP, box, tilt, flags)
        if nseg > 2:
            o = o.copy()
            o[nseg // 2] = -1                      # one segment without an oxygen
        cls = RC.mixed_classes(nseg)               # prolines among them
        per_layout = []
        for offsets in SC.layouts(nseg):
            det = []
            want = R.classes(coords, tuple(box) + tuple(tilt), n, ca, c, o, offsets, cls, flags, det)
            per_layout.append((offsets, want, det))
        _SWEEP[key] = (coords, (n, ca, c, o), cls, per_layout)
    return _SWEEP[key]


def size_edges(lib, cell, device=False):
    """every nseg x range layout in one cell, bit-identical to the restatement with no value left out: batch_frames unset / 1 / 3, and a
    scratch bound that forces sub-batches of one frame"""
    box, tilt, flags = CELLS[cell]
    for nseg in NSEG:
        coords, (n, ca, c, o), cls, per_layout = sweep_case(cell, nseg)
        for offsets, want, det in per_layout:
            what = f"nseg {nseg}, ranges {len(offsets) - 1}, tilt {tilt}, flags {flags}"
            ir = ss_ir(lib, n, ca, c, o, offsets, cls)
            for batch in (0, 1, 3):
                with Option(lib, "batch_frames", batch):
                    check(TG.evaluate(lib, ir, coords, box, tilt=tilt, flags=flags, device=device), want, det, f"{what}: batch_frames {batch}")
            with Option(lib, "ss_scratch_bytes", 1):
                check(TG.evaluate(lib, ir, coords, box, tilt=tilt, flags=flags, device=device), want, det, f"{what}: one frame of scratch")
    assert lib.vmd_set_option(b"ss_scratch_bytes", 256 << 20) == 256 << 20        # the default, and every override above was undone


@pytest.mark.parametrize("cell", range(len(CELLS)))
def test_size_edges_on_the_emulator(emu_lib, cell):
    size_edges(emu_lib, cell)


def test_the_sweep_covers_what_it_must():
    """a condition on the INPUTS, asserted on the restatement's output: every code at least 20 times, a parallel and an antiparallel
    ladder whose partner indices straddle 63 | 64 and 127 | 128, a turn whose bond crosses 63 | 64, a bridge between two ranges"""
    total = np.zeros(9, np.int64)
    par, anti, turns, cross = set(), set(), 0, 0
    for cell in range(len(CELLS)):
        for nseg in NSEG:
            _, _, _, per_layout = sweep_case(cell, nseg)
            for offsets, want, det in per_layout:
                total += np.bincount(want.ravel(), minlength=9)
                rng = R.ranges_of(nseg, offsets)
                for d in det:
                    P, A = d["par"], d["anti"]
                    for e in (63, 127):
                        if nseg > e + 1:
                            if (P[:-1, e] & P[1:, e + 1]).any():
                                par.add(e)
                            if (A[:-1, e + 1] & A[1:, e]).any():
                                anti.add(e)
                    for k in (3, 4, 5):
                        i = np.flatnonzero(d["turn"][k])
                        turns += int(((i < 64) & (i + k >= 64)).sum())
                    i, j = np.nonzero(P | A)
                    cross += int((rng[i] != rng[j]).sum())
    print("codes 0..8:", total.tolist(), "parallel", sorted(par), "antiparallel", sorted(anti), "turns over 63|64:", turns, "bridges between ranges:", cross)
    assert total[0] == 0 and (total[1:] >= 20).all()
    assert par == {63, 127} and anti == {63, 127} and turns >= 1 and cross >= 1


# ---- 3. inputs at the thresholds -------------------------------------------------------------------------------------------------------

def _threshold_z():
    """the O ... N distance along z at which the planted geometry has E = -0.5 exactly (bisection in fp64)"""
    energy = lambda z: 27.888 * (1.0 / z + 1.0 / (z + 0.23) - 1.0 / (z - 1.0) - 1.0 / (z + 1.23))
    lo, hi = 2.9, 6.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if energy(mid) < -0.5 else (lo, mid)
    return lo


def threshold_case():
    """eight segments in one range on a 20 A lattice in a 50 A cell; the bond 1 -> 4 is the only one, a 3-turn that makes 2 and 3 TURN.
    Frames 0 .. 12: the O of segment 1 moves along z through E = -0.5; frames 13 .. 25: E = -2.9 and CA[1] moves through 9 A of CA[4]"""
    z0 = _threshold_z()
    steps = np.array([-0.3, -1e-2, -1e-4, -3e-6, -1e-6, -3e-7, 0.0, 3e-7, 1e-6, 3e-6, 1e-4, 1e-2, 0.3])
    F = 2 * steps.size
    site = np.array([(20.0 * (s & 1), 20.0 * ((s >> 1) & 1), 20.0 * (s >> 2)) for s in range(8)]) + 3.0
    xyz = np.zeros((F, 32, 3))
    for f in range(F):
        N = site.copy()
        O = N + np.array([3.1, 2.7, -4.2])
        CA = N + np.array([1.2, 0.8, 0.3])
        if f < steps.size:
            O[1] = N[4] + np.array([0.0, 0.0, z0 + steps[f]])
            CA[1] = CA[4] + np.array([4.0, 0.0, 0.0])
        else:
            O[1] = N[4] + np.array([0.0, 0.0, 2.9])
            CA[1] = CA[4] + np.array([9.0 + steps[f - steps.size], 0.0, 0.0])
        xyz[f, 0::4], xyz[f, 1::4], xyz[f, 2::4], xyz[f, 3::4] = N, CA, O + np.array([0.0, 0.0, 1.23]), O
    box = (50.0, 50.0, 50.0)
    return SC.frames_of(xyz, box, shift=(-4.0, -4.0, -4.0)), box, SC.backbone(8), steps.size


def near_thresholds(lib, device=False):
    coords, box, (n, ca, c, o), half = threshold_case()
    det = []
    want = R.classes(coords, box, n, ca, c, o, [0, 8], details=det)
    e = np.array([d["energy"][1, 4] for d in det[:half]])
    g = np.array([d["gate2"][1, 4] for d in det[half:]])
    print("E:", e.tolist(), "CA^2:", g.tolist())
    assert (e < -0.5).any() and (e >= -0.5).any() and np.abs(e + 0.5).min() < 1e-5          # both sides of the energy, closely
    assert (g < 81.0).any() and (g >= 81.0).any() and np.abs(g - 81.0).min() < 1e-3         # both sides of the gate, closely
    assert all(set(zip(*np.nonzero(d["evaluated"]))) <= {(1, 4), (4, 1)} for d in det)      # no other pair passes a gate
    bonded = np.array([bool(d["hb"][1, 4]) for d in det])
    assert bonded.any() and not bonded.all()
    assert all((want[f, 2:4] == R.TURN).all() == bonded[f] for f in range(len(det)))         # the class row shows the bond
    check(TG.evaluate(lib, ss_ir(lib, n, ca, c, o, [0, 8]), coords, box, device=device), want, det, "thresholds")


def test_near_thresholds_on_the_emulator(emu_lib):
    near_thresholds(emu_lib)


# ---- 4. IR validation, fingerprint, atoms, the oxygens of a topology -------------------------------------------------------------------

def _bb(n=(0, 4, 8), ca=(1, 5, 9), c=(2, 6, 10), o=(3, 7, 11), offsets=(0, 3), cls=None):
    return dict(n=n, ca=ca, c=c, o=o, offsets=offsets, cls=cls)


BAD = [(_bb(n=(), ca=(), c=(), o=(), offsets=(0,)), "no segment"),
       (_bb(ca=(1, -5, 9)), "negative atom index"),
       (_bb(offsets=(1, 3)), "start at 0"),
       (_bb(offsets=(0, 2, 2, 3)), "must increase"),
       (_bb(offsets=(0, 2)), "end at"),
       (_bb(cls=(0, 4, 255)), "class 4"),
       (_bb(o=(3, -2, 11)), "O list holds -2 for segment 1"),
       (_bb(o=None), "no carbonyl oxygen list")]


@pytest.mark.parametrize("args,msg", BAD)
def test_ir_validation_errors(host_lib, args, msg):
    ir = V.ScriptIR(host_lib)
    with pytest.raises(V.VmdError, match=msg):
        ir.add_secondary_structure(NAMES, **args)
    assert ir.property_count() == 0


def test_ir_validation_of_size_names_and_null(host_lib):
    import ctypes as C
    ir = V.ScriptIR(host_lib)
    big = np.arange(L.SS_MAX_SEGMENTS + 1, dtype=np.int32)
    with pytest.raises(V.VmdError, match="at most 16384"):
        ir.add_secondary_structure(NAMES, big, big, big, big, [0, big.size])
    ir.add_secondary_structure(("a", "b"), big[:-1], big[:-1], big[:-1], big[:-1], [0, big.size - 1])      # the limit itself is accepted
    ir.add_distance("d", [0], [1])
    for names, msg in ((("d", "m"), "already defined"), (("t", "d"), "already defined"), (("t", "t"), "already defined"), (("", "m"), "empty")):
        with pytest.raises(V.VmdError, match=msg):
            ir.add_secondary_structure(names, **_bb())
    two = (C.c_char_p * 2)(b"t", b"m")
    idx = (C.c_int32 * 3)(0, 1, 2)
    off = (C.c_uint32 * 2)(0, 3)
    good = L.BackboneC(3, idx, idx, idx, 1, off, None)
    assert not host_lib.vmd_ir_add_secondary_structure(ir.h, two, None, idx) and "backbone" in host_lib.last_error()
    assert not host_lib.vmd_ir_add_secondary_structure(ir.h, None, C.byref(good), idx)
    assert not host_lib.vmd_ir_add_secondary_structure(None, two, C.byref(good), idx)
    assert not host_lib.vmd_ir_add_secondary_structure(ir.h, two, C.byref(good), None) and "oxygen" in host_lib.last_error()
    for field in ("n", "ca", "c", "range_offsets"):
        bad = L.BackboneC(3, idx, idx, idx, 1, off, None)
        setattr(bad, field, None)
        assert not host_lib.vmd_ir_add_secondary_structure(ir.h, two, C.byref(bad), idx), field
    assert ir.property_count() == 3
    assert host_lib.vmd_ir_add_secondary_structure(ir.h, two, C.byref(good), idx) and ir.property_names() == ["a", "b", "d", "t", "m"]


def test_fingerprint_work_and_atoms(host_lib):
    def fp(**kw):
        ir = V.ScriptIR(host_lib)
        ir.add_secondary_structure(NAMES, **_bb(**kw))
        return ir.fingerprint()
    base = fp()
    assert base == fp() and base == fp(cls=(0, 0, 0))                 # NULL classes: no proline
    assert base != fp(n=(0, 4, 7)) and base != fp(ca=(1, 5, 12)) and base != fp(c=(3, 6, 10))
    assert base != fp(o=(3, 7, 12)) and base != fp(o=(3, -1, 11)) and fp(o=(3, -1, 11)) != fp(o=(-1, 7, 11))
    assert base != fp(offsets=(0, 1, 3)) and base != fp(offsets=(0, 2, 3)) and fp(offsets=(0, 1, 3)) != fp(offsets=(0, 2, 3))
    assert base != fp(cls=(0, 0, 2)) and fp(cls=(0, 0, 2)) != fp(cls=(0, 2, 0))
    # not the fingerprint of the ramachandran statement over the same backbone and names
    ir = V.ScriptIR(host_lib)
    ir.add_ramachandran(NAMES, (0, 4, 8), (1, 5, 9), (2, 6, 10), (0, 3))
    assert ir.fingerprint() != base
    ir = V.ScriptIR(host_lib)
    ir.add_distance("d", [0, 1], [2, 3, 4])
    w0 = int(host_lib.vmd_ir_work_per_frame(ir.h))
    ir.add_secondary_structure(NAMES, **_bb(o=(3, -1, 11)))
    assert int(host_lib.vmd_ir_work_per_frame(ir.h)) == w0 + 3 * 3 // 8 + 4 * 3
    assert list(ir.geometry_atoms("ss")) == [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11] and list(ir.geometry_atoms("ss", 0)) == [0, 1, 2, 3]
    assert list(ir.geometry_atoms("ss", 1)) == [4, 5, 6] and ir.geometry_atoms("ss", 3).size == 0 and ir.geometry_atoms("sspop").size == 0


def test_an_oxygen_outside_the_trajectory_is_refused(emu_lib):
    coords = np.zeros((1, 3, 12), np.float32)
    ir = ss_ir(emu_lib, **_bb(o=(3, -1, 12)))
    ev = V.ScriptEval(1, ir)
    cell = V.make_unitcell(30.0)
    with pytest.raises(V.VmdError, match="references atom 12"):
        ev.frame_range(V.MolSystem(12, unitcell=cell), V.HostTrajectory(coords, cell), 0, 1)


def test_backbone_oxygens_of_a_topology(host_lib):
    """ALA with O | GLY whose O comes behind an OT1 (O wins) | a terminal residue with OT1 and OT2 | one with O1 | one with OC1 | one with none"""
    res = [("ALA", ["N", "CA", "C", "O", "CB"]), ("GLY", ["N", "CA", "C", "OT1", "O"]), ("ALA", ["N", "CA", "C", "OT2", "OT1"]),
           ("ALA", ["N", "CA", "C", "O1", "O2"]), ("ALA", ["N", "CA", "OC1", "C"]), ("ALA", ["N", "CA", "C", "OXT"]), ("HOH", ["O", "H", "H"])]
    names, resn, ri = [], [], []
    for r, (rn, atoms) in enumerate(res):
        names += atoms
        resn += [rn] * len(atoms)
        ri += [r] * len(atoms)
    topo = script.Topology([a[0] for a in names], resn, ri, names=names)
    bb = script.backbone_from_topology(topo)
    assert bb["n"].size == 6
    py = script.backbone_oxygens_from_topology(topo, bb)
    assert py.dtype == np.int32 and list(py) == [3, 9, 14, 18, 22, -1]
    cc = script.backbone_oxygens_from_topology_native(topo, bb, lib=host_lib)
    assert cc.dtype == np.int32 and np.array_equal(py, cc)
    ir = V.ScriptIR(host_lib)
    ir.add_secondary_structure(NAMES, bb["n"], bb["ca"], bb["c"], py, bb["range_offsets"], bb["rama_class"])
    assert ir.property_count() == 2
    assert host_lib.vmd_topology_backbone_oxygens(None, None, None, 0) == 0 and "NULL" in host_lib.last_error()


def test_exporters(emu_lib, tmp_path):
    xyz = SC.ideal(-57.0, -47.0, 6)
    n, ca, c, o = SC.backbone(6)
    ev = TG.evaluate(emu_lib, ss_ir(emu_lib, n, ca, c, o, [0, 6]), np.repeat(SC.frames_of(xyz, BIG), 2, axis=0), BIG)
    for name, last in (("ss", 6), ("sspop", 9)):
        path = tmp_path / f"{name}.csv"
        ev.export_table(path, name, fmt="csv")
        assert f"{name}[{last}]" in path.read_text() and f"{name}[{last + 1}]" not in path.read_text()


# ---- 5. next to the other forms ----------------------------------------------------------------------------------------------------------

def next_to_the_other_forms(lib, oracle, device=False):
    """VIAMD's default script plus a ramachandran statement, with and without a secondary_structure statement in the same IR: every other
    property is bit-identical, and the new one equals the restatement"""
    atoms, blob, box, F = 6001, 200, 30.0, 20
    coords, topo = TG.blob_system(oracle, n_atoms=atoms, n_blob=blob, box=box, F=F, seed=5)
    names = np.array(["N", "CA", "C", "O", "CB", "H", "HA", "HB1", "CG", "HG"])
    topo.names = np.where(np.arange(atoms) < blob, names[np.arange(atoms) % 10], topo.elements)
    bb = script.backbone_from_topology(topo)
    o = script.backbone_oxygens_from_topology(topo, bb)
    assert bb["n"].size == blob // 10 and (o == bb["n"] + 3).all()
    evs = []
    for with_ss in (False, True):
        ir = script.compile_script_native(TG.VIAMD_DEFAULT_SCRIPT, topo, lib=lib, **OPT_INS)
        ir.add_ramachandran(("bb", "rama"), **bb)
        if with_ss:
            ir.add_secondary_structure(NAMES, bb["n"], bb["ca"], bb["c"], o, bb["range_offsets"], bb["rama_class"])
        evs.append(TG.evaluate(lib, ir, coords, box, topo.mass, device=device))
    plain, both = evs
    props = plain.ir.property_names()
    assert props == ["d1", "a1", "r", "v", "lin", "plan", "iso", "bb", "rama"] and both.ir.property_names() == props + list(NAMES)
    for name in props:
        a, b = plain.property_data(name), both.property_data(name)
        assert a.dim == b.dim and a.fingerprint == b.fingerprint, name
        assert np.array_equal(a.values.view(np.int32), b.values.view(np.int32)), name
        if a.c.counts:
            assert np.array_equal(a.counts, b.counts), name
    det = []
    want = R.classes(coords, box, bb["n"], bb["ca"], bb["c"], o, bb["range_offsets"], bb["rama_class"], details=det)
    check(both, want, det, "blob")


def test_next_to_the_other_forms_on_the_emulator(emu_lib, oracle):
    next_to_the_other_forms(emu_lib, oracle)


# ---- 6. call patterns and the merge -------------------------------------------------------------------------------------------------------

def pattern_case(frames=7):
    box = CELLS[0][0]
    coords, (n, ca, c, o), _ = SC.planted(77, 66, frames, box)
    return box, coords, (n, ca, c, o), [0, 33, 66]


def call_patterns(lib, device=False):
    """the call patterns of test_rama.call_patterns: frame by frame, uneven ranges, pool threads (read-ahead), clear_data and again; and a
    filtered eval that takes its blocks from a source eval"""
    box, coords, (n, ca, c, o), offsets = pattern_case()
    F = coords.shape[0]
    ir = ss_ir(lib, n, ca, c, o, offsets)
    one = TG.evaluate(lib, ir, coords, box, device=device)
    want = (classes(one), pops(one))
    assert np.array_equal(want[0], R.classes(coords, box, n, ca, c, o, offsets)) and len(np.unique(want[0])) >= 5
    for kw in (dict(ranges=[(f, f + 1) for f in range(F)]), dict(ranges=[(0, 3), (3, 6), (6, 7)]), dict(pooled=(4, 2))):
        ev = TG.evaluate(lib, ir, coords, box, device=device, **kw)
        assert np.array_equal(classes(ev), want[0]) and np.array_equal(pops(ev), want[1]), kw
    cell = V.make_unitcell(box)
    import cases
    sysm, traj = V.MolSystem(coords.shape[2], unitcell=cell), cases.make_traj(lib, coords, cell, device)
    # a source eval evaluated in blocks of two frames; a second eval takes frames 2 .. 5 out of its blocks
    src = V.ScriptEval(F, ir)
    src.set_block_frames(2)
    assert src.frame_range(sysm, traj, 0, F)
    flt = V.ScriptEval(F, ir)
    flt.set_block_frames(2)
    flt.set_source(src)
    assert flt.frame_range(sysm, traj, 2, 6)
    assert np.array_equal(classes(src), want[0]) and np.array_equal(classes(flt)[2:6], want[0][2:6]) and np.array_equal(pops(flt)[2:6], want[1][2:6])
    assert not classes(flt)[:2].any() and not classes(flt)[6:].any() and flt.frame_stats()[1] > 0
    # clear_data followed by a second evaluation gives the same result
    one.clear_data()
    assert not classes(one).any() and not pops(one).any()
    assert one.frame_range(sysm, traj, 0, F)
    assert np.array_equal(classes(one), want[0]) and np.array_equal(pops(one), want[1])


def test_call_patterns_on_the_emulator(emu_lib):
    call_patterns(emu_lib)


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
    box, coords, (n, ca, c, o), offsets = pattern_case(frames=8)
    F = coords.shape[0]
    ev = V.ScriptEval(F, ss_ir(lib, n, ca, c, o, offsets))
    beg, end = shard_frames(F, rank, world)
    cell = V.make_unitcell(box)
    assert ev.frame_range(V.MolSystem(coords.shape[2], unitcell=cell), V.HostTrajectory(coords, cell), beg, end)
    own = classes(ev)
    reduce_eval(ev)
    assert ev.frame_mask().all()
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), own=own, t=classes(ev), p=pops(ev), beg=beg, end=end)
    dist.destroy_process_group()


def test_two_rank_merge(emu_lib, tmp_path):
    """two evals over halves of 8 frames, merged through the host collective: the merged table is the union of the ranks' rows and equals
    one eval over all frames"""
    import torch.multiprocessing as mp
    port = 45500 + (os.getpid() % 2000)
    mp.spawn(_merge_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    box, coords, (n, ca, c, o), offsets = pattern_case(frames=8)
    one = TG.evaluate(emu_lib, ss_ir(emu_lib, n, ca, c, o, offsets), coords, box)
    union = np.zeros_like(classes(one))
    for r in range(2):
        z = np.load(tmp_path / f"rank{r}.npz")
        beg, end = int(z["beg"]), int(z["end"])
        assert np.array_equal(z["own"][beg:end], classes(one)[beg:end]) and not np.delete(z["own"], np.s_[beg:end], axis=0).any()
        union += z["own"]
        assert np.array_equal(z["t"], classes(one)) and np.array_equal(z["p"], pops(one))
    assert np.array_equal(union, classes(one)) and classes(one).all()
