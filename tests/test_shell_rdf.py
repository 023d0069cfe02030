"""rdf() over within() shells on the emulator build and in the host-only entry points: known answers, exactness at the shell
radius, pencil == masked all-pairs == the yardstick (tests/shell_rdf_ref.py) on the 12 001-atom blob system in three kinds of cell,
identities that need no yardstick, the DECISION switches, call patterns, a pencil-bucket overflow, co-evaluation with static rdfs, a
two-rank merge, export, the opt-in front-end (C++ and Python twin), ABI validation and VIAMD's default script plus a shell rdf line
through the shim.  Histogram counts are integers: every comparison of them is `==`; weights64 to 1e-12 relative (fp64 sums in another
order)."""
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

import shell_rdf_ref as S
import within_ref as W
import test_geometry as TG
import test_within as TW
from test_within import options, launches, evaluate, TILT, blob12k, sets_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIAMD_DEFAULT_SCRIPT = TG.VIAMD_DEFAULT_SCRIPT
GS_LINE = "\ngs = rdf(element('O') and within(3.5, resname(\"ALA\")), element('O'), 8.0);"
PENCIL_KEYS = ("shell_flags", "shell_compact", "rdf_pencil")
BRUTE_KEYS = ("shell_brute", "rdf_brute")


def make_ir(lib, props):
    """props: [(name, (T, shell | None), (T, shell | None), rmin, rmax)], shell = (R, r_min, r_max)"""
    ir = V.ScriptIR(lib)
    for name, a, b, rmin, rmax in props:
        ir.add_rdf_shell(name, a[0], b[0], (rmin, rmax), ref_shell=a[1], target_shell=b[1])
    return ir


def run(lib, props, coords, box, **kw):
    return evaluate(lib, make_ir(lib, props), coords, box, **kw)


def profiled(lib, fn, force_brute=0):
    lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
    try:
        with options(lib, force_brute=force_brute):
            out = fn()
    finally:
        lib.vmd_profile_enable(False)
    return out, {k: launches(lib, k) for k in PENCIL_KEYS + BRUTE_KEYS + ("cells_build",)}


def both_paths(lib, props, coords, box, **kw):
    """the evaluator with and without a grid, asserted from the profile counters -> (pencil eval, all-pairs eval, pencil counters)"""
    ev_p, n_p = profiled(lib, lambda: run(lib, props, coords, box, **kw))
    assert all(n_p[k] >= 1 for k in PENCIL_KEYS) and all(n_p[k] == 0 for k in BRUTE_KEYS), n_p
    ev_b, n_b = profiled(lib, lambda: run(lib, props, coords, box, **kw), force_brute=1)
    assert all(n_b[k] >= 1 for k in BRUTE_KEYS) and all(n_b[k] == 0 for k in PENCIL_KEYS), n_b
    for name, *_ in props:
        a, b = ev_p.property_data(name), ev_b.property_data(name)
        assert np.array_equal(a.counts, b.counts), name
        assert np.array_equal(a.weights64, b.weights64), name          # the same host arithmetic on the same populations
    return ev_p, ev_b, n_p


def check(lib, O, ev, name, want, rmin, rmax):
    """the record of an rdf, against the yardstick's (counts, weights64)"""
    counts, weights = want[0], want[1]
    pd = ev.property_data(name)
    assert tuple(pd.dim[:3]) == (1, 1, 1024) and pd.unit_str == ("Å", "")
    assert pd.min_range[0] == np.float32(rmin) and pd.max_range[0] == np.float32(rmax)
    np.testing.assert_array_equal(pd.counts, counts, err_msg=f"{name}: integer histogram differs from the yardstick")
    np.testing.assert_allclose(pd.weights64, weights, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(pd.values, counts.astype(np.float32))
    if weights.sum() > 0:
        g_dev = V.downsample_histogram(pd.values, pd.weights, 128, lib=lib)
        g_ref = O.downsample_histogram(counts.astype(np.float32), weights.astype(np.float32), 128)
        np.testing.assert_allclose(g_dev, g_ref, rtol=1e-5, atol=0)


def varied(pops, nt):
    """the non-saturation rule, on the YARDSTICK's populations: neither empty nor full in any frame, and not all equal"""
    pops = np.asarray(pops)
    assert ((pops > 0) & (pops < nt)).all() and (len(pops) == 1 or len(set(pops.tolist())) > 1), (pops, nt)


def total(ev, name):
    return int(np.asarray(ev.property_data(name).counts).sum())


# ---- 1. known answers ------------------------------------------------------------------------------------------------------------------

def known_answers(lib, O, device=False):
    kw = dict(device=device)
    # R = atom 0; t = atom 1 sits 3.0 away from it exactly; B = atoms 2 - 4, two of them within 2.0 of t, one 10 away
    pts = [(10.0, 10.0, 10.0), (13.0, 10.0, 10.0), (14.0, 10.0, 10.0), (13.0, 11.5, 10.0), (23.0, 10.0, 10.0)]
    xyz = np.asarray(pts, np.float32).T.copy()[None]
    B = [2, 3, 4]

    def pairs(rlo, rhi, closed=0):
        with options(lib, spec_within_closed=closed):
            evs = both_paths(lib, [("g", ([1], ([0], rlo, rhi)), (B, None), 0.0, 2.0)], xyz, 50.0, **kw)
        want = S.shell_rdf(O, xyz, 50.0, [([1], ([0], rlo, rhi)), (B, None)], 0.0, 2.0, closed=bool(closed))
        assert total(evs[0], "g") == total(evs[1], "g") == int(want[0].sum())
        check(lib, O, evs[0], "g", want, 0.0, 2.0)
        return total(evs[0], "g")
    assert pairs(0.0, 3.0) == 0                                                     # open above: t is out, none of its pairs counted
    assert pairs(0.0, float(np.nextafter(np.float32(3.0), np.float32(4.0)))) == 2   # t is in: exactly its two pairs
    assert pairs(3.0, 5.0) == 2                                                     # closed below
    assert pairs(0.0, 3.0, closed=1) == 2
    # the same on the target side, and with both sides shells
    ev = run(lib, [("g", (B, None), ([1], ([0], 3.0, 5.0)), 0.0, 2.0), ("h", ([1], ([0], 0.0, 4.0)), (B, ([1], 0.0, 1.2)), 0.0, 2.0)], xyz, 50.0, **kw)
    assert total(ev, "g") == 2 and total(ev, "h") == 1                               # h: of B only atom 2 is within 1.2 of atom 1
    # an empty shell in every frame: zeros, never an error
    ev = run(lib, [("g", ([1], ([0], 0.0, 1.0)), (B, None), 0.0, 2.0)], xyz, 50.0, **kw)
    pd = ev.property_data("g")
    assert not np.asarray(pd.counts).any() and not np.asarray(pd.weights64).any()
    # an atom in both sides meets itself at d = 0: dropped by the open interval, counted once under spec_rdf_closed
    rng = np.random.default_rng(3)
    cloud = rng.uniform(0.0, 20.0, (300, 3)).astype(np.float32).T.copy()[None]
    every = np.arange(300, dtype=np.int32)
    sides = [(every, (every, 0.5, 1.5)), (every, (every, 0.5, 1.5))]
    res = {}
    for closed in (0, 1):
        old = O.set_spec("rdf_closed", closed)
        try:
            with options(lib, spec_rdf_closed=closed):
                evs = both_paths(lib, [("g", sides[0], sides[1], 0.0, 4.0)], cloud, 20.0, **kw)
            want = S.shell_rdf(O, cloud, 20.0, sides, 0.0, 4.0)
        finally:
            O.set_spec("rdf_closed", old)
        varied(want[2][0], 300)
        check(lib, O, evs[0], "g", want, 0.0, 4.0)
        res[closed] = (np.asarray(evs[0].property_data("g").counts).copy(), int(want[2][0][0]))
    diff = res[1][0].astype(np.int64) - res[0][0].astype(np.int64)
    assert diff[0] == res[0][1] and not diff[1:].any()                               # one pair (i, i) per member, all in the bin of d = 0


def test_known_answers_on_the_emulator(emu_lib, oracle):
    known_answers(emu_lib, oracle)


RADII = [1.0, 3.5, 1.0 / 3.0, 7.25, 2.0 ** 0.5]


def radius_exactness(lib, O, device=False, radii=RADII):
    """shell atoms whose distance from the one reference atom steps through the floats around r: each is in or out exactly as the yardstick
    says, and brings exactly its pairs with it"""
    checked = 0
    for r in radii:
        r = np.float32(r)
        step = TW.steps(r)
        pts = [(0.0, 0.0, 0.0)] + [(x, 0.0, 0.0) for x in step] + [(x, np.float32(0.8) * r, 0.0) for x in TW.steps(np.float32(0.6) * r)]
        n = len(pts)
        # one partner 0.25 r above every stepping atom: the eight atoms of a group lie within a few ulps of each other, so each of them has
        # the group's eight partners within the pair cutoff 0.3 r and nothing else (the other group is more than 0.8 r away)
        partners = [(p[0], p[1], np.float32(0.25) * r) for p in pts[1:]]
        xyz = np.asarray(pts + partners, np.float32).T.copy()[None]
        box = float(np.float32(12.0) * r)
        B = np.arange(n, xyz.shape[2], dtype=np.int32)
        cut = float(np.float32(0.3) * r)
        props = [(f"s{t}", ([t], ([0], 0.0, float(r))), (B, None), 0.0, cut) for t in range(1, n)] + \
                [(f"r{t}", ([t], ([0], float(r), float(np.float32(2.0) * r))), (B, None), 0.0, cut) for t in range(1, n)]
        for closed in (0, 1):
            with options(lib, spec_within_closed=closed):
                ev = run(lib, props, xyz, box, device=device)
                with options(lib, force_brute=1):
                    evb = run(lib, props, xyz, box, device=device)
            ins = []
            for name, a, b, lo, hi in props:
                want = S.shell_rdf(O, xyz, box, [a, b], lo, hi, closed=bool(closed))
                assert np.array_equal(ev.property_data(name).counts, want[0]) and np.array_equal(evb.property_data(name).counts, want[0]), (float(r), closed, name)
                assert int(want[0].sum()) == 8 * int(want[2][0][0]), (float(r), name)    # in: exactly its eight pairs; out: nothing
                if name[0] == "s":
                    ins.append(int(want[2][0][0]))
            assert 0 < sum(ins[:8]) < 8, (float(r), ins)                              # the steps along x do straddle the radius
            checked += 1
    return checked


def test_radius_exactness_on_the_emulator(emu_lib, oracle):
    assert radius_exactness(emu_lib, oracle) == 2 * len(RADII)


# ---- 2. the blob system: pencil == masked all pairs == yardstick ---------------------------------------------------------------------------

POPULATIONS = {"a": [920, 927, 933], "b": [1916, 1933, 1904], "c": [1793, 1795, 1792], "e": [3255, 3245, 3222]}


def blob_shells(s):
    """the shells of test_within.BLOB_SCRIPT"""
    return {"a": (s["wo"], (s["blob"], 0.0, 3.5)), "b": (s["wo"], (s["wo"], 0.5, 2.0)), "c": (s["wo"], (s["h"], 1.2, 1.8)),
            "e": (s["water"], (s["blob"], 2.0, 4.0))}


def blob_props(s):
    sh = blob_shells(s)
    return [("ref_shell", sh["a"], (s["wo"], None), 0.0, 6.0),                 # a shell as the reference argument
            ("tgt_shell", (s["blob"], None), sh["b"], 0.0, 6.0),               # ... as the target argument
            ("both", sh["a"], sh["c"], 0.5, 5.0),                              # both sides
            ("wide_shell", sh["e"], (s["wo"], None), 0.0, 3.0),                # shell radius 4.0 above the pair cutoff 3.0
            ("shared", sh["a"], (s["h"], None), 0.0, 6.0)]                     # the shell of ref_shell again


def on_the_blob(lib, O, device=False, cells=None):
    coords, topo = blob12k(O, 3)
    s = sets_of(topo)
    props = blob_props(s)
    cells = cells or [dict(box=50.0), dict(box=(50.0, 50.0, 50.0), tilt=TILT), dict(box=50.0, flags=3)]
    for cell in cells:
        tri = "tilt" in cell
        # the tilted cell restricts the YARDSTICK to frame 0 (as kernels_on_the_blob does: its all-pairs arithmetic has no slab shortcut
        # there); the product then evaluates frame 0 alone as well, so that nothing it computes is left out of the comparison
        frames = [0] if tri else [0, 1, 2]
        cc = coords[:1] if tri else coords
        evs = both_paths(lib, props, cc, cell["box"], device=device, **{k: v for k, v in cell.items() if k != "box"})
        n_compared = 0
        for name, a, b, lo, hi in props:
            want = S.shell_rdf(O, cc, cell["box"], [a, b], lo, hi, tilt=cell.get("tilt", (0.0, 0.0, 0.0)), flags=cell.get("flags", 7), frames=frames)
            assert want[2].shape == (2, len(frames))
            for k, side in enumerate((a, b)):
                if side[1] is not None:
                    varied(want[2][k], len(side[0]))
            assert want[0].sum() > 0
            for ev in evs[:2]:
                check(lib, O, ev, name, want, lo, hi)
            n_compared += 1
        assert n_compared == len(props)
    # the populations the issue lists, orthorhombic cell, frames 0 - 2
    sh = blob_shells(s)
    for k, v in sh.items():
        pops = S.shell_rdf(O, coords, 50.0, [v, (s["blob"][:1], None)], 0.0, 1.0)[2][0]
        assert pops.tolist() == POPULATIONS[k], (k, pops)
    # two properties sharing one shell cost no more walks than one of them
    _, n_two = profiled(lib, lambda: run(lib, [props[0], props[4]], coords, 50.0, device=device))
    _, n_one = profiled(lib, lambda: run(lib, [props[0]], coords, 50.0, device=device))
    assert n_two["shell_flags"] == n_one["shell_flags"] >= 1 and n_two["shell_compact"] == n_one["shell_compact"], (n_one, n_two)
    assert n_two["rdf_pencil"] == 2 * n_one["rdf_pencil"]


def test_pencil_brute_and_yardstick_on_the_blob_system(emu_lib, oracle):
    on_the_blob(emu_lib, oracle)


# ---- 3. identities that need no yardstick ------------------------------------------------------------------------------------------------

def identities(lib, O, device=False):
    import cases
    coords = cases.water_box(O, 2, 3000, 31.0, 4)
    o, h = cases.oxygen(3000), cases.hydrogen(3000)
    # R = T, r_min = 0: every atom is within 0 of itself, H = T, and the record is the static rdf's bit for bit
    ir = V.ScriptIR(lib)
    ir.add_rdf("static", o, h, (0.5, 7.0))
    ir.add_rdf_shell("shell", o, h, (0.5, 7.0), ref_shell=(o, 0.0, 2.0))
    ir.add_rdf_shell("shell_t", o, h, (0.5, 7.0), target_shell=(h, 0.0, 0.1))
    ev = evaluate(lib, ir, coords, 31.0, device=device)
    st = ev.property_data("static")
    for name in ("shell", "shell_t"):
        pd = ev.property_data(name)
        assert np.array_equal(pd.counts, st.counts) and np.array_equal(np.asarray(pd.weights64).view(np.int64), np.asarray(st.weights64).view(np.int64)), name
        assert TG.bits_equal(pd.values, st.values) and TG.bits_equal(pd.weights, st.weights)
    assert np.asarray(st.counts).sum() > 0
    # the weights of g are the shell populations the count property reports, frame by frame
    coords, topo = TG.blob_system(O, n_atoms=3000, n_blob=200, F=6)
    text = ("nw = count(water and element('O') and within(3.5, not water));"
            "g = rdf(water and element('O') and within(3.5, not water), element('H'), 1.0:6.0);")
    irs, info = script.compile_script(text, topo, lib=lib, within=True, shell_rdf=True)
    ev = evaluate(lib, irs, coords, 30.0, device=device)
    nw = TG.rows(ev, "nw")[:, 0].astype(np.float64)
    assert len(set(nw.tolist())) > 1 and (nw > 0).all()
    nB = len(info["g"]["target"])
    want = sum(n * nB / 30.0 ** 3 * (4.0 / 3.0) * math.pi * (6.0 ** 3 - 1.0 ** 3) for n in nw)
    got = float(np.asarray(ev.property_data("g").weights64).sum())
    assert abs(got - want) <= 1e-12 * want, (got, want)


def test_identities(emu_lib, oracle):
    identities(emu_lib, oracle)


# ---- 4. the DECISION switches -----------------------------------------------------------------------------------------------------------

def switch_system():
    """300 atoms in a 40 A cell; atom 150 sits 3.0 from atom 0 exactly and nothing else comes within 4.5 of atom 0"""
    rng = np.random.default_rng(11)
    p = rng.uniform(0.0, 40.0, (300, 3)).astype(np.float32)
    p[0] = (5.0, 5.0, 5.0)
    d = np.linalg.norm(p - p[0], axis=1)
    p[(d < 4.5) & (np.arange(300) > 0)] += np.float32(15.0)
    p[150] = (8.0, 5.0, 5.0)
    frames = np.stack([p, p + rng.normal(0.0, 0.3, p.shape).astype(np.float32)])
    frames[1, 0], frames[1, 150] = p[0], p[150]
    return np.ascontiguousarray(frames.transpose(0, 2, 1))


def switches(lib, O, device=False):
    xyz = switch_system()
    T, R, B = np.arange(0, 200, dtype=np.int32), np.arange(100, 300, dtype=np.int32), np.arange(0, 300, dtype=np.int32)
    sides = [(T, (R, 0.0, 3.0)), (B, None)]
    props = [("g", sides[0], sides[1], 0.0, 6.0)]

    def product(**opt):
        with options(lib, **opt):
            ev = both_paths(lib, props, xyz, 40.0, device=device)[0]
        pd = ev.property_data("g")
        return ev, np.asarray(pd.counts).copy(), np.asarray(pd.weights64).copy()

    def yardstick(closed=False, exclude_ref=False, shell_norm=False, **spec):
        old = {k: O.set_spec(k, v) for k, v in spec.items()}
        try:
            return S.shell_rdf(O, xyz, 40.0, sides, 0.0, 6.0, closed=closed, exclude_ref=exclude_ref, shell_norm=shell_norm)
        finally:
            for k, v in old.items():
                O.set_spec(k, v)
    ev0, c0, w0 = product()
    base = yardstick()
    varied(base[2][0], 200)
    check(lib, O, ev0, "g", base, 0.0, 6.0)
    cases_ = [(dict(spec_within_closed=1), dict(closed=True), "counts"),
              (dict(spec_within_exclude_ref=1), dict(exclude_ref=True), "counts"),
              (dict(spec_rdf_closed=1), dict(rdf_closed=1), "counts"),
              (dict(spec_rdf_norm=1), dict(rdf_norm=1), "weights"),
              (dict(spec_rdf_norm=2), dict(rdf_norm=2), "weights"),
              (dict(spec_shell_norm=1), dict(shell_norm=True), "weights"),
              (dict(spec_shell_norm=1, spec_rdf_norm=2, spec_within_closed=1), dict(shell_norm=True, rdf_norm=2, closed=True), "counts")]
    for opt, ykw, moves in cases_:
        ev, c, w = product(**opt)
        want = yardstick(**ykw)
        check(lib, O, ev, "g", want, 0.0, 6.0)
        # the switch is live on this input: the result differs from the default's (counts never depend on the two norm switches)
        if moves == "counts":
            assert not np.array_equal(c, c0), opt
        else:
            assert np.array_equal(c, c0) and not np.allclose(w, w0, rtol=1e-9, atol=0), opt
    # spec_within_closed lets atom 0 in (its one reference atom sits at d == r_max exactly)
    assert yardstick(closed=True)[2][0][0] == base[2][0][0] + 1


def test_switches(emu_lib, oracle):
    switches(emu_lib, oracle)


# ---- 5. call patterns --------------------------------------------------------------------------------------------------------------------

CALL_SCRIPT = ("g = rdf(water and element('O') and within(3.5, not water), element('O'), 6.0); s = rdf(element('O'), element('O'), 6.0);"
               "b = rdf(element('O') and within(0.5:2.9, element('O')), element('H') and within(4.0, not water), 1.0:5.0); d = distance(10, 30);"
               "nw = count(water and element('O') and within(3.5, not water));")
CALL_NAMES = ("g", "s", "b")
RAGGED = [(0, 7), (7, 8), (8, 21), (21, 30)]


def same_rdf(ev, ref, names=CALL_NAMES, what=""):
    for name in names:
        a, b = ev.property_data(name), ref.property_data(name)
        assert np.array_equal(a.counts, b.counts), (what, name)
        np.testing.assert_allclose(a.weights64, b.weights64, rtol=1e-12, atol=0, err_msg=f"{what} {name}")
        assert np.asarray(b.counts).sum() > 0 and np.asarray(b.weights64).sum() > 0


def call_patterns(lib, O, device=False):
    import cases
    coords, topo = TG.blob_system(O, n_atoms=3000, n_blob=200, F=30)
    ir, info = script.compile_script(CALL_SCRIPT, topo, lib=lib, within=True, shell_rdf=True)
    runit = lambda **kw: evaluate(lib, ir, coords, 30.0, device=device, **kw)
    one_call = runit()
    want = S.shell_rdf(O, coords, 30.0, [(info["g"]["ref"], tuple(info["g"]["ref_shell"][k] for k in ("ref", "rmin", "rmax"))),
                                          (info["g"]["target"], None)], 0.0, 6.0)
    varied(want[2][0], len(info["g"]["ref"]))
    check(lib, O, one_call, "g", want, 0.0, 6.0)
    assert np.array_equal(TG.rows(one_call, "nw")[:, 0], want[2][0].astype(np.float32))      # |H(f)| is what count() reports, always
    got = {"frame by frame": runit(ranges=[(f, f + 1) for f in range(30)]), "grain 1": runit(pooled=(16, 1)), "grain 4": runit(pooled=(4, 4)),
           "ragged": runit(ranges=RAGGED), "late first": runit(ranges=RAGGED[::-1])}
    for bf in (3, 16):
        with options(lib, batch_frames=bf):
            got[f"batch_frames {bf}"] = runit()
    with options(lib, batch_frames=4, defer_sync=0):
        got["no deferred sync"] = runit()
    with options(lib, readahead=0):
        got["no read-ahead"] = runit(pooled=(8, 1))
    with options(lib, force_brute=1):
        got["all pairs"] = runit()
    if lib.vmd_device_count() > 0:
        got["resident" if not device else "host"] = evaluate(lib, ir, coords, 30.0, device=not device)
    # block partials, and a second eval served from them over a sub-range
    full = V.ScriptEval(30, ir); full.set_block_frames(5)
    cell = V.make_unitcell(30.0)
    sysm, traj = V.MolSystem(coords.shape[2], unitcell=cell), cases.make_traj(lib, coords, cell, device)
    assert full.frame_range(sysm, traj, 0, 30)
    got["block partials"] = full
    for what, ev in got.items():
        same_rdf(ev, one_call, what=what)
        assert TG.bits_equal(TG.rows(ev, "nw"), TG.rows(one_call, "nw")), what
    filt = V.ScriptEval(30, ir); filt.set_source(full)
    assert filt.frame_range(sysm, traj, 5, 22)
    assert filt.frame_stats()[1] > 0
    direct = V.ScriptEval(30, ir)
    assert direct.frame_range(sysm, traj, 5, 22)
    same_rdf(filt, direct, what="filtered from block partials")
    assert not np.array_equal(direct.property_data("g").counts, one_call.property_data("g").counts)
    # the block partials of a read-ahead: pooled calls against an eval that keeps blocks
    ahead = V.ScriptEval(30, ir); ahead.set_block_frames(5)
    assert ahead.frame_range_pooled(sysm, traj, 0, 30, 8, 1)
    same_rdf(ahead, one_call, what="pooled with block partials")
    # a cutoff above half the cell: choose_grid fails, that property alone goes through the masked all-pairs path
    o = np.nonzero(np.asarray(topo.elements) == "O")[0].astype(np.int32)
    blob = np.arange(200, dtype=np.int32)
    props = [("wide", (o, (blob, 0.0, 3.5)), (o, None), 0.0, 16.0), ("near", (o, (blob, 0.0, 3.5)), (o, None), 0.0, 6.0)]
    ev, n = profiled(lib, lambda: run(lib, props, coords[:2], 30.0, device=device))
    assert n["shell_brute"] >= 1 and n["rdf_brute"] >= 1 and n["shell_flags"] >= 1 and n["rdf_pencil"] >= 1, n
    for name, a, b, lo, hi in props:
        check(lib, O, ev, name, S.shell_rdf(O, coords[:2], 30.0, [a, b], lo, hi), lo, hi)
    # spec_rdf_raw acts on the pair histogram only: the shell is the wrapped one
    far = coords[:2].copy(); far[:, :, ::7] += np.float32(60.0)
    old = O.set_spec("rdf_raw", 1)
    try:
        with options(lib, spec_rdf_raw=1):
            ev, n = profiled(lib, lambda: run(lib, props[1:], far, 30.0, device=device))
        assert n["shell_brute"] >= 1 and n["shell_flags"] == 0
        check(lib, O, ev, "near", S.shell_rdf(O, far, 30.0, [props[1][1], props[1][2]], 0.0, 6.0), 0.0, 6.0)
    finally:
        O.set_spec("rdf_raw", old)


def test_call_patterns(emu_lib, oracle):
    call_patterns(emu_lib, oracle)


# ---- 6. a pencil-bucket overflow ------------------------------------------------------------------------------------------------------------

def overflow_case(lib, O, device=False):
    """the construction of test_within.overflow_case: the middle frames pile every oxygen into one pencil, a bucket sized from the batch's
    ends overflows, and the batch - walk, compaction and pass - is repeated"""
    import cases
    n, box, F = 3000, 60.0, 12
    coords = cases.water_box(O, 5, n, box, F)
    o, h = cases.oxygen(n), cases.hydrogen(n)
    rng = np.random.default_rng(3)
    for f in (5, 6, 7):
        coords[f][:, o] = rng.uniform(1.0, 11.0, (3, o.size)).astype(np.float32)
    R = np.concatenate([o[::100], h[::50]])     # a few oxygens that sit in the pile, and hydrogens that mark their own oxygen everywhere else
    props = [("n", (o, (R, 0.5, 2.5)), (o, None), 0.0, 5.0), ("m", (h, None), (o, (R, 0.5, 2.0)), 0.0, 5.0)]
    want = {nm: S.shell_rdf(O, coords, box, [a, b], lo, hi) for nm, a, b, lo, hi in props}
    varied(want["n"][2][0], o.size)
    varied(want["m"][2][1], o.size)
    with options(lib, cells_small=0, cells_cap_sample=2):
        for bf, defer in ((0, 1), (4, 1), (4, 0)):
            with options(lib, batch_frames=bf, defer_sync=defer):
                ev = run(lib, props, coords, box, device=device)
                assert ev.cell_build_stats()[0] >= 1, (bf, defer)
                for nm, a, b, lo, hi in props:
                    check(lib, O, ev, nm, want[nm], lo, hi)


def test_a_bucket_overflow_repeats_walk_compaction_and_pass(emu_lib, oracle):
    overflow_case(emu_lib, oracle)


# ---- 7. co-evaluation, multi-rank, export ----------------------------------------------------------------------------------------------------

C5_SCRIPT = ("goo = rdf(element('O'), element('O'), 8.0); ghv = rdf(not element('H'), not element('H'), 8.0);"
             "gbw = rdf(not water, water and element('O'), 8.0);")
C5_SHELL = "gsh = rdf(water and element('O') and within(3.5, not water), not element('H'), 8.0);"


def coevaluation(lib, O, device=False):
    coords, topo = TG.blob_system(O, n_atoms=3000, n_blob=200, F=4)
    ev0, n0 = profiled(lib, lambda: evaluate(lib, script.compile_script(C5_SCRIPT, topo, lib=lib)[0], coords, 30.0, device=device))
    ir1, info = script.compile_script(C5_SCRIPT + C5_SHELL, topo, lib=lib, shell_rdf=True)
    ev1, n1 = profiled(lib, lambda: evaluate(lib, ir1, coords, 30.0, device=device))
    assert n1["rdf_pencil"] == n0["rdf_pencil"] + 1 and n0["rdf_pencil"] >= 3          # the classes of the static rdfs are untouched
    for name in ("goo", "ghv", "gbw"):
        a, b = ev0.property_data(name), ev1.property_data(name)
        assert np.array_equal(a.counts, b.counts) and np.asarray(a.counts).sum() > 0, name
        assert np.array_equal(np.asarray(a.weights64).view(np.int64), np.asarray(b.weights64).view(np.int64)), name
        assert TG.bits_equal(a.values, b.values) and TG.bits_equal(a.weights, b.weights), name
    i = info["gsh"]
    want = S.shell_rdf(O, coords, 30.0, [(i["ref"], (i["ref_shell"]["ref"], i["ref_shell"]["rmin"], i["ref_shell"]["rmax"])), (i["target"], None)], 0.0, 8.0)
    varied(want[2][0], len(i["ref"]))
    check(lib, O, ev1, "gsh", want, 0.0, 8.0)


def test_static_rdfs_are_unchanged_by_a_shell_line(emu_lib, oracle):
    coevaluation(emu_lib, oracle)


MERGE_SCRIPT = "g = rdf(water and element('O') and within(3.5, not water), element('O'), 6.0); d = distance(10, 30);"


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
    coords, topo = TG.blob_system(O, n_atoms=3000, F=7)
    ir = script.compile_script(MERGE_SCRIPT, topo, lib=lib, shell_rdf=True)[0]
    F = coords.shape[0]
    ev = V.ScriptEval(F, ir)
    beg, end = shard_frames(F, rank, world)
    cell = V.make_unitcell(30.0)
    assert ev.frame_range(V.MolSystem(coords.shape[2], unitcell=cell), V.HostTrajectory(coords, cell), beg, end)
    reduce_eval(ev)
    assert ev.frame_mask().all()
    pd = ev.property_data("g")
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), counts=np.asarray(pd.counts), weights64=np.asarray(pd.weights64), values=np.asarray(pd.values))
    dist.destroy_process_group()


def test_two_rank_merge_equals_the_single_evaluation(emu_lib, oracle, tmp_path):
    import torch.multiprocessing as mp
    port = 41500 + (os.getpid() % 2000)
    mp.spawn(_merge_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    coords, topo = TG.blob_system(oracle, n_atoms=3000, F=7)
    ir = script.compile_script(MERGE_SCRIPT, topo, lib=emu_lib, shell_rdf=True)[0]
    pd = evaluate(emu_lib, ir, coords, 30.0).property_data("g")
    assert np.asarray(pd.counts).sum() > 0
    for r in range(2):
        z = np.load(tmp_path / f"rank{r}.npz")
        assert np.array_equal(z["counts"], pd.counts) and TG.bits_equal(z["values"], pd.values)
        np.testing.assert_allclose(z["weights64"], pd.weights64, rtol=1e-12, atol=0)


def test_export_table(emu_lib, oracle, tmp_path):
    coords, topo = TG.blob_system(oracle, n_atoms=3000, F=5)
    ir = script.compile_script(MERGE_SCRIPT, topo, lib=emu_lib, shell_rdf=True)[0]
    ev = evaluate(emu_lib, ir, coords, 30.0)
    ir0 = script.compile_script("g = rdf(water and element('O'), element('O'), 6.0);", topo, lib=emu_lib)[0]
    ev0 = evaluate(emu_lib, ir0, coords, 30.0)
    for ext in ("xvg", "csv"):
        path, path0 = tmp_path / f"g.{ext}", tmp_path / f"g0.{ext}"
        ev.export_table(path, "g", ext)
        ev0.export_table(path0, "g", ext)
        text, text0 = open(path, encoding="utf-8").read(), open(path0, encoding="utf-8").read()
        nums = [ln.replace(",", " ").split() for ln in text.splitlines() if ln.strip() and ln.strip()[0] in "0123456789"]
        nums0 = [ln.replace(",", " ").split() for ln in text0.splitlines() if ln.strip() and ln.strip()[0] in "0123456789"]
        assert "g" in text and len(nums) == len(nums0) > 0                     # the table of an rdf: the same rows as the static one's
        assert [ln[0] for ln in nums] == [ln[0] for ln in nums0]
        y = np.array([float(ln[1]) for ln in nums])
        assert np.isfinite(y).all() and y.max() > 0 and [ln[1] for ln in nums] != [ln[1] for ln in nums0]


# ---- 8. front-end ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def topo():
    return synth.water_box_topology(200 + 933 * 3, n_blob=200)


OPT_INS = dict(angles=True, shape=True, rmsd=True, within=True)


def test_without_the_opt_in_nothing_changes(host_lib, topo):
    import test_rmsd
    assert test_rmsd._old_ir(host_lib).fingerprint() == test_rmsd.PARENT_FINGERPRINT          # the literal the parent's suite holds
    text = VIAMD_DEFAULT_SCRIPT + TW.NW_LINE + GS_LINE
    ir_a, rep_a = script.compile_script_native(text, topo, lib=host_lib, partial=True, **OPT_INS)
    ir_b, rep_b = script.compile_script_native(text, topo, lib=host_lib, partial=True, shell_rdf=False, **OPT_INS)
    ir_py, _, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, shell_rdf=False, **OPT_INS)
    assert ir_a.property_names() == ir_b.property_names() == ir_py.property_names() == ["d1", "a1", "r", "v", "lin", "plan", "iso", "nw"]
    assert ir_a.fingerprint() == ir_b.fingerprint() == ir_py.fingerprint() and rep_a == rep_b == rep_py
    k = rep_a["skipped"][0]
    assert [s["names"] for s in rep_a["skipped"]] == ["gs"] and text[k["beg"]:k["end"]] == GS_LINE[1:-1]
    assert k["reason"] == "unsupported function 'within' (outside the rdf / sdf / distance path)"      # the parent commit's words
    assert GS_LINE[1:] in rep_a["fallback_source"]
    # scripts without the form keep their fingerprints and reports whatever the new bit says
    for text0, kw in ((VIAMD_DEFAULT_SCRIPT, OPT_INS), (VIAMD_DEFAULT_SCRIPT, {}), (VIAMD_DEFAULT_SCRIPT + TW.NW_LINE, OPT_INS),
                      ("x = within(3, all); v = sdf(resname(\"ALA\"), within(3, all), 5.0); g = rdf(all, element('O'), 2.0:5.0); d = distance(1, 2);", {})):
        res = [script.compile_script_native(text0, topo, lib=host_lib, partial=True, shell_rdf=w, **kw) for w in (False, True)]
        res.append(script.compile_script(text0, topo, lib=host_lib, partial=True, shell_rdf=True, **kw)[::2])
        assert len({r[0].fingerprint() for r in res}) == 1 and res[0][1] == res[1][1] == res[2][1], text0
    # a static rdf compiled with the bit is the ir vmd_ir_add_rdf builds
    q = V.ScriptIR(host_lib); q.add_rdf("g", np.arange(2999), np.nonzero(np.asarray(topo.elements) == "O")[0], (2.0, 5.0))
    q2 = V.ScriptIR(host_lib); q2.add_rdf_shell("g", np.arange(2999), np.nonzero(np.asarray(topo.elements) == "O")[0], (2.0, 5.0))
    assert q.fingerprint() == q2.fingerprint() == script.compile_script_native("g = rdf(all, element('O'), 2.0:5.0);", topo, lib=host_lib, shell_rdf=True).fingerprint()
    for compiler in (script.compile_script_native, script.compile_script):
        with pytest.raises(script.ScriptError) as err:
            compiler(GS_LINE[1:], topo, lib=host_lib, **OPT_INS)
        assert str(err.value) == "unsupported function 'within' (outside the rdf / sdf / distance path)"


def test_default_script_with_the_shell_line(host_lib, topo):
    text = VIAMD_DEFAULT_SCRIPT + GS_LINE
    kw = dict(angles=True, shape=True, shell_rdf=True)
    ir_c, rep_c = script.compile_script_native(text, topo, lib=host_lib, partial=True, **kw)
    ir_py, info, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, **kw)
    assert ir_c.property_names() == ir_py.property_names() == ["d1", "a1", "r", "v", "lin", "plan", "iso", "gs"]
    assert ir_c.fingerprint() == ir_py.fingerprint() and ir_c.property_flags("gs") == ir_c.property_flags("r")
    assert rep_c == rep_py and rep_c["skipped"] == []
    fb = rep_c["fallback_source"]
    assert len(fb) == len(text) and fb.strip() == 's1 = resname("ALA")[2:8];'
    i = info["gs"]
    assert i["kind"] == "rdf" and i["target_shell"] is None and (i["rmin"], i["rmax"]) == (0.0, 8.0)
    assert (i["ref_shell"]["rmin"], i["ref_shell"]["rmax"]) == (0.0, 3.5) and list(i["ref_shell"]["ref"]) == list(range(200))
    assert len(i["ref"]) == len(i["target"]) == 20 + 933
    assert ir_c.geometry_atoms("gs").size == 0                                       # as for every rdf
    assert int(host_lib.vmd_ir_work_per_frame(ir_c.h)) - int(host_lib.vmd_ir_work_per_frame(
        script.compile_script_native(VIAMD_DEFAULT_SCRIPT, topo, lib=host_lib, angles=True, shape=True).h)) == 953 * 953 + 953 + 200
    strict = script.compile_script_native(text, topo, lib=host_lib, **kw)
    assert strict.fingerprint() == ir_c.fingerprint()


# (statement, |T_ref|, ref shell (|R|, a, b) or None, |T_tgt|, tgt shell or None)
ACCEPTED = [
    ("g = rdf(within(3.5, resname(\"ALA\")), water, 5.0);", 2999, (200, 0.0, 3.5), 2799, None),
    ("g = rdf(water, within(3.5:5.0, protein) and water, 5.0);", 2799, None, 2799, (200, 3.5, 5.0)),
    ("g = rdf(water and within(2, atom(1:30)) and element('O'), element('O') and within(0.5:2.0, element('O')), {1.0, 6.0});", 933, (30, 0.0, 2.0), 953, (953, 0.5, 2.0)),
    ("g = rdf((element('O') or element('N')) and not water and within(1.5, (water)), all, 4.0);", 40, (2799, 0.0, 1.5), 2999, None),
    ("s = resname(\"ALA\")[2:8]; w = water and element('O'); g = rdf(w and within(0.5:2.5, s), w, 2.0:7.0);", 933, (70, 0.5, 2.5), 933, None),
]

SKIPPED = [
    ("g = rdf(water and not within(3, protein), water, 5.0);", "within() must be a factor of the top-level AND"),
    ("g = rdf(water or within(3, protein), water, 5.0);", "within() must be a factor of the top-level AND"),
    ("g = rdf(water, water and (within(3, protein)), 5.0);", "within() must be a factor of the top-level AND"),
    ("g = rdf(within(3, protein) and within(5, water), water, 5.0);", "an rdf argument takes exactly one within() factor, found 2"),
    ("g = rdf(water and within(3, within(4, protein)), water, 5.0);", "an rdf argument takes exactly one within() factor, found 2"),
    ("g = sdf(resname(\"ALA\"), within(3, protein), 5.0);", "unsupported function 'within'"),
    ("g = distance(within(3, protein), water);", "unsupported function 'within'"),
    ("g = rdf(resname(\"XYZ\") and within(3, protein), water, 5.0);", "g: empty selection"),
    ("g = rdf(water and within(3, resname(\"XYZ\")), water, 5.0);", "g: empty selection"),
    ("g = rdf(water and within(0, protein), water, 5.0);", "within needs a radius > 0"),
    ("g = rdf(water, water and within(5:3, protein), 5.0);", "within range needs 0 <= a < b"),
    ("g = rdf(water and within(3:3, protein), water, 5.0);", "within range needs 0 <= a < b"),
    ("g = rdf(water and within(3), water, 5.0);", "expected ,"),
    ("g = rdf(water and within(protein, 3), water, 5.0);", "expected num"),
    ("g = rdf(within(3), water, 5.0);", "expected ,"),
    ("d = rdf(water and within(3, protein), water, 5.0);", "already defined"),
]


@pytest.mark.parametrize("stmt,nta,sha,ntb,shb", ACCEPTED)
def test_accepted_forms(host_lib, topo, stmt, nta, sha, ntb, shb):
    ir_c = script.compile_script_native(stmt, topo, lib=host_lib, shell_rdf=True)
    ir_py, info = script.compile_script(stmt, topo, lib=host_lib, shell_rdf=True)
    assert ir_c.property_names() == ir_py.property_names() == ["g"] and ir_c.fingerprint() == ir_py.fingerprint()
    i = info["g"]
    assert (len(i["ref"]), len(i["target"])) == (nta, ntb)
    work = nta * ntb
    for got, want, nt in ((i["ref_shell"], sha, nta), (i["target_shell"], shb, ntb)):
        assert (got is None) == (want is None)
        if want:
            assert (len(got["ref"]), got["rmin"], got["rmax"]) == want
            work += nt + want[0]
    assert int(host_lib.vmd_ir_work_per_frame(ir_c.h)) == work
    assert ir_c.geometry_atoms("g").size == 0
    # the statement without its within() factors is another ir
    assert ir_c.fingerprint() != script.compile_script_native("g = rdf(water, water, 5.0);", topo, lib=host_lib, shell_rdf=True).fingerprint()


@pytest.mark.parametrize("stmt,reason", SKIPPED)
def test_skipped_forms(host_lib, topo, stmt, reason):
    text = "d = distance(1, 2);\n" + stmt + "\ne = distance(3, 4);"
    for compiler in (script.compile_script_native, script.compile_script):
        with pytest.raises((script.ScriptError, V.VmdError)) as err:
            compiler(text, topo, lib=host_lib, shell_rdf=True)
        assert reason in str(err.value)
    ir_c, rep_c = script.compile_script_native(text, topo, lib=host_lib, partial=True, shell_rdf=True)
    ir_py, _, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, shell_rdf=True)
    assert ir_c.property_names() == ir_py.property_names() == ["d", "e"] and ir_c.fingerprint() == ir_py.fingerprint()
    assert rep_c == rep_py and len(rep_c["skipped"]) == 1
    k = rep_c["skipped"][0]
    assert k["names"] == stmt.split(" ")[0] and reason in k["reason"] and text[k["beg"]:k["end"]] == stmt[:-1]
    assert stmt in rep_c["fallback_source"] and "distance(3, 4)" not in rep_c["fallback_source"]


# ---- 9. ABI --------------------------------------------------------------------------------------------------------------------------------

def test_ir_validation_errors(host_lib):
    lib = host_lib
    for sym in ("vmd_ir_add_rdf_shell", "vmd_hip_within_brute_flags", "vmd_hip_within_pencil_flags", "vmd_hip_shell_compact", "vmd_hip_rdf_brute_masked"):
        assert hasattr(lib, sym), sym
    ir = V.ScriptIR(lib)
    ok = dict(ref_shell=([1], 0.0, 3.0))
    for a, b, cut, kw, msg in (([], [1], 5.0, ok, "rdf reference set is empty"), ([0], [], 5.0, ok, "rdf target set is empty"), ([0, -1], [1], 5.0, ok, "negative"),
                               ([0], [1], (3.0, 3.0), ok, "0 <= rmin < rmax"), ([0], [1], 5.0, dict(ref_shell=([], 0.0, 3.0)), "within reference set is empty"),
                               ([0], [1], 5.0, dict(target_shell=([-2], 0.0, 3.0)), "negative"),
                               ([0], [1], 5.0, dict(ref_shell=([1], 3.0, 3.0)), "within range must be finite and satisfy 0 <= rmin < rmax"),
                               ([0], [1], 5.0, dict(target_shell=([1], -1.0, 3.0)), "0 <= rmin < rmax"),
                               ([0], [1], 5.0, dict(ref_shell=([1], 0.0, float("inf"))), "finite"),
                               ([0], [1], 5.0, dict(ref_shell=ok["ref_shell"], target_shell=([1], float("nan"), 3.0)), "finite")):
        with pytest.raises(V.VmdError, match=msg):
            ir.add_rdf_shell("g", a, b, cut, **kw)
    with pytest.raises(V.VmdError, match="name is empty"):
        ir.add_rdf_shell("", [0], [1], 5.0, **ok)
    assert ir.property_count() == 0
    ir.add_distance("d", [0], [1])
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_rdf_shell("d", [0], [1], 5.0, **ok)
    ir.add_rdf_shell("g", [0, 5, 7], [1, 5], (0.5, 3.0), ref_shell=([2, 3, 4, 5], 0.0, 2.0), target_shell=([9], 1.0, 2.0))
    assert ir.property_names() == ["d", "g"] and ir.property_flags("g") == L.FLAG_DISTRIBUTION
    assert ir.geometry_atoms("g").size == 0
    assert int(lib.vmd_ir_work_per_frame(ir.h)) == 1 + 3 * 2 + (3 + 4) + (2 + 1)

    def fp(*args, **kw):
        q = V.ScriptIR(lib)
        q.add_rdf_shell(*args, **kw)
        return q.fingerprint()
    base = ("g", [0, 1, 2], [3, 4], (0.0, 3.0))
    sh = ([5, 6], 0.0, 2.0)
    fps = [fp(*base), fp(*base, ref_shell=sh), fp(*base, target_shell=sh), fp(*base, ref_shell=sh, target_shell=sh), fp(*base, ref_shell=([5], 0.0, 2.0)),
           fp(*base, ref_shell=([5, 6], 0.5, 2.0)), fp(*base, ref_shell=([5, 6], 0.0, 2.5)), fp("h", *base[1:], ref_shell=sh)]
    q = V.ScriptIR(lib); q.add_rdf(*base)
    assert fps[0] == q.fingerprint() and len(set(fps)) == len(fps)
    ir2 = V.ScriptIR(lib)
    ir2.add_rdf_shell("g", [0, 1], [1], 3.0, ref_shell=([99], 0.0, 3.0))
    if lib.vmd_device_count() > 0:
        with pytest.raises(V.VmdError, match="references atom 99"):
            TG.evaluate(lib, ir2, np.zeros((1, 3, 10), np.float32), 10.0)


# ---- 10. VIAMD's default script plus a shell rdf line through the shim ----------------------------------------------------------------------

def build_shim_shell_rdf():
    """tests/native/shim_default_script_shell_rdf.cpp linked against the product library"""
    return native_host.build_shim("shim_default_script_shell_rdf")


def test_shim_default_script_with_the_shell_line_on_the_emulator(emu_lib, tmp_path):
    import conftest
    exe = native_host.build_shim("shim_default_script_shell_rdf", conftest.build_emu(), tmp_path / "shim_shell_rdf_emu")
    native_host.run_ok([exe, "8"], "OK frames=8 properties=8 gs=gpu fallback_frame_range_calls=0")
    out = native_host.run_ok([exe, "8", "nobit"], "OK frames=8 properties=8 gs=fallback")
    assert "fallback_frame_range_calls=0" not in out.stdout, out.stdout
