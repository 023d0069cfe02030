"""and / or / not over within() shells on the emulator build and in the host-only entry points: known answers for all sixteen
tables of two terms, the six expressions of the 12 001-atom blob system in three kinds of cell on the walk, on all pairs and under the
rule that mixes both, the kernels' size edges, identities that need no yardstick, a pencil-bucket overflow, call patterns, co-evaluation,
a two-rank merge, the opt-in front-end (C++ and Python twin), ABI validation, vmd_eval_shell_mask and VIAMD's default script plus a
bridging count and a second-shell sdf through the shim.  The yardstick is tests/shell_expr_ref.py.  Counts, masks, populations and
voxels are integers: every comparison is `==`."""
import functools
import os
import sys

import numpy as np
import pytest

import native_host

import viamd_amd as V
from viamd_amd import _lib as L
from viamd_amd import script, synth

import shell_expr_ref as X
import within_ref as W
import test_geometry as TG
import test_within as TW
import test_shell_sdf as TS
from test_geometry import rows, bits_equal
from test_within import options, launches, evaluate, TILT, blob12k, sets_of, varied
from test_shell_sdf import vol, caps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("shell_expr", "shell_expr_brute", "shell_expr_finish")
BITS = dict(within=True, shell_sdf=True, shell_expr=True)
FOUR = X.table(lambda a, b, c, d: a and b and not c and d, 4)


def profiled(lib, fn, **opt):
    lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
    try:
        with options(lib, **opt):
            out = fn()
    finally:
        lib.vmd_profile_enable(False)
    return out, {k: launches(lib, k) for k in KEYS + ("batches", "cells_build")}


def count_ir(lib, props):
    """props: [(name, T, terms, truth)]"""
    ir = V.ScriptIR(lib)
    for name, t, terms, truth in props:
        ir.add_within_count_expr(name, t, terms, truth)
    return ir


def count_rows(lib, props, coords, box, **kw):
    ev = evaluate(lib, count_ir(lib, props), coords, box, **kw)
    out = {}
    for name, *_ in props:
        pd = ev.property_data(name)
        assert tuple(pd.dim[:2]) == (coords.shape[0], 1) and pd.unit_str == ("", "")          # the record of a within count
        out[name] = rows(ev, name)[:, 0]
    return out


# ---- 1. known answers ------------------------------------------------------------------------------------------------------------------

def known_answers(lib, device=False):
    """twelve atoms in a box of 50: R0 = atom 0 at x = 10, R1 = atom 1 at x = 14 (also an entry of T: it meets itself at d = 0), the other
    entries of T near both, near one, near none, and atom 6 at 3.0 from R0 exactly.  Frame 1 moves both reference atoms away: every
    h is 0 except atom 1's own.  h_0 and h_1 are written down by hand; all sixteen tables are asked at once."""
    pts = np.array([(10, 10, 10), (14, 10, 10), (12, 10, 10), (16.5, 10, 10), (8, 10, 10), (30, 30, 30), (10, 13, 10), (12, 11, 10),
                    (30, 10, 10), (12, 10, 11), (40, 40, 40), (8, 11, 10)], np.float64)
    f1 = pts.copy(); f1[0] = (45, 45, 20); f1[1] = (45, 45, 30)
    xyz = np.ascontiguousarray(np.stack([pts, f1]).astype(np.float32).transpose(0, 2, 1))
    T = np.array([2, 3, 4, 5, 6, 1, 7, 8, 9, 10, 11], np.int32)
    terms = [([0], 0.0, 3.0), ([1], 0.0, 3.0)]
    props = [(f"t{tt}", T, terms, tt) for tt in range(16)]
    bx = X.as_box(50.0)
    for closed in (0, 1):
        for excl in (0, 1):
            #          atom:  2  3  4  5  6       1  7  8  9  10 11
            h0 = np.array([1, 0, 1, 0, closed, 0, 1, 0, 1, 0, 1])
            h1 = np.array([1, 1, 0, 0, 0, 1 - excl, 1, 0, 1, 0, 0])
            g1 = np.array([0, 0, 0, 0, 0, 1 - excl, 0, 0, 0, 0, 0])            # frame 1
            hand = {tt: [int(X.lookup(h0 + 2 * h1, tt, 2).sum()), int(X.lookup(2 * g1, tt, 2).sum())] for tt in range(16)}
            want = {tt: X.counts(xyz, bx, T, terms, tt, closed=bool(closed), exclude_ref=bool(excl)) for tt in range(16)}
            for tt in range(16):
                assert want[tt].tolist() == hand[tt], (closed, excl, tt, want[tt], hand[tt])
            # the empty frame, the boundary and the self rule do show in these numbers
            assert hand[X.AND2][1] == 0 and hand[X.AND2][0] == 3 and hand[X.A_NOT_B][0] == 2 + closed
            assert hand[X.table(lambda a, b: not b, 2)][0] == 6 + excl
            for opt in (dict(), dict(shell_brute_below=0), dict(force_brute=1)):
                for skip in (1, 0):
                    with options(lib, spec_within_closed=closed, spec_within_exclude_ref=excl, shell_expr_skip=skip, **opt):
                        got = count_rows(lib, props, xyz, 50.0, device=device)
                    for tt in range(16):
                        assert got[f"t{tt}"].tolist() == hand[tt], (closed, excl, opt, skip, tt, got[f"t{tt}"], hand[tt])
                        assert not np.signbit(got[f"t{tt}"]).any()                    # a frame with no member is +0


def test_known_answers_on_the_emulator(emu_lib):
    known_answers(emu_lib)


# ---- 2. the six expressions of the blob system ---------------------------------------------------------------------------------------------

def blob_exprs(s):
    """name -> (positions in the pool of terms, truth); the pool: A, B, the whole blob at 5.0, S, the water oxygens at 0.5:2.8"""
    blob, wo = s["blob"], s["wo"]
    pool = [(blob[:600], 0.0, 3.5), (blob[1000:1600], 0.0, 3.5), (blob, 0.0, 5.0), (blob[:300], 0.0, 6.0), (wo, 0.5, 2.8)]
    ex = {"n_and": ((0, 1), X.AND2), "n_anb": ((0, 1), X.A_NOT_B), "n_xor": ((0, 1), X.XOR2), "n_or": ((0, 1), X.OR2),
          "bulk": ((2,), X.NOT1), "four": ((3, 0, 1, 4), FOUR)}
    return pool, ex


BLOB_SCRIPT = ("n_and = count(water and element('O') and within(3.5, atom(1:600)) and within(3.5, atom(1001:1600)));\n"
               "n_anb = count(water and element('O') and within(3.5, atom(1:600)) and not within(3.5, atom(1001:1600)));\n"
               "n_xor = count(water and element('O') and ((within(3.5, atom(1:600)) and not within(3.5, atom(1001:1600))) or "
               "(not within(3.5, atom(1:600)) and within(3.5, atom(1001:1600)))));\n"
               "n_or = count(water and element('O') and (within(3.5, atom(1:600)) or within(3.5, atom(1001:1600))));\n"
               "bulk = count(water and element('O') and not within(5.0, not water));\n"
               "four = count(water and element('O') and within(6.0, atom(1:300)) and within(3.5, atom(1:600)) and "
               "not within(3.5, atom(1001:1600)) and within(0.5:2.8, water and element('O')));")
CELLS = {"cubic": dict(box=50.0), "tilted": dict(box=(50.0, 50.0, 50.0), tilt=TILT), "slab": dict(box=50.0, flags=3)}
# the populations DESIGN 1.9 records for the cubic cell, checked against the yardstick below
CUBIC_POPS = {"n_and": [3, 6, 10, 14], "n_anb": [275, 280, 290, 289], "n_xor": [617, 621, 632, 618], "n_or": [620, 627, 642, 632],
              "bulk": [1933, 1965, 1951, 1970], "four": [141, 139, 151, 156]}


@functools.lru_cache(maxsize=None)
def _blob_reference(O, cell):
    """the yardstick's rows, once per session and cell: every term of the pool through within_ref.hits once per frame.  The tilted cell
    has no slab shortcut - all pairs in numpy: two frames there, and the term over the 3 334 water oxygens themselves on frame 0 only"""
    coords, topo = blob12k(O, 4)
    s = sets_of(topo)
    pool, ex = blob_exprs(s)
    c = CELLS[cell]
    bx = X.as_box(c["box"], c.get("tilt", (0.0, 0.0, 0.0)), c.get("flags", 7))
    frames = [0, 1] if cell == "tilted" else [0, 1, 2, 3]
    out = {k: [] for k in ex}
    for f in frames:
        cheap = cell == "tilted" and f > 0
        idx = X.outcomes(coords[f], bx, s["wo"], pool[:4] if cheap else pool)
        for k, (w, tr) in ex.items():
            if not (cheap and 4 in w):
                out[k].append(int(X.lookup(X.select(idx, w), tr, len(w)).sum()))
    return {k: np.asarray(v, np.float32) for k, v in out.items()}


def blob_reference(O, cell):
    want = _blob_reference(O, cell)
    nt = 3334
    for k, w in want.items():                # the non-saturation rule, on the yardstick's numbers, before anything is compared
        if len(w) > 1:
            varied(w, nt)
        else:
            assert 0 < w[0] < nt
    if cell == "cubic":
        assert {k: w.astype(int).tolist() for k, w in want.items()} == CUBIC_POPS
    return want


def blob_props(s):
    pool, ex = blob_exprs(s)
    return [(k, s["wo"], [pool[i] for i in w], tr) for k, (w, tr) in ex.items()]


def on_the_blob(lib, O, device=False, cells=("cubic", "tilted", "slab")):
    coords, topo = blob12k(O, 4)
    s = sets_of(topo)
    props = blob_props(s)
    # 13 term passes: four expressions of two terms, one of one, one of four (S = blob[:300] is the one list below shell_brute_below)
    settings = {"walk": (dict(shell_brute_below=0), (13, 0, 6)), "all pairs": (dict(force_brute=1), (0, 13, 6)), "rule": (dict(), (12, 1, 6))}
    for cell in cells:
        want = blob_reference(O, cell)
        c = CELLS[cell]
        cc = coords[:2] if cell == "tilted" else coords
        kw = {k: v for k, v in c.items() if k != "box"}
        for what, (opt, n_want) in settings.items():
            res = []
            for skip in (1, 0):
                got, n = profiled(lib, lambda: count_rows(lib, props, cc, c["box"], device=device, **kw), shell_expr_skip=skip, **opt)
                assert n["batches"] == 1 and tuple(n[k] for k in KEYS) == n_want, (cell, what, skip, n)
                assert (n["cells_build"] >= 1) == (what != "all pairs"), (cell, what, n)
                for k in want:
                    assert np.array_equal(got[k][:len(want[k])], want[k]), (cell, what, skip, k, got[k], want[k])
                res.append(got)
            for k in res[0]:
                assert np.array_equal(res[0][k], res[1][k]), (cell, what, k)          # shell_expr_skip changes no row


def test_the_blob_expressions_cubic(emu_lib, oracle):
    on_the_blob(emu_lib, oracle, cells=("cubic",))


def test_the_blob_expressions_tilted(emu_lib, oracle):
    on_the_blob(emu_lib, oracle, cells=("tilted",))


def test_the_blob_expressions_slab(emu_lib, oracle):
    on_the_blob(emu_lib, oracle, cells=("slab",))


def twins_on_the_blob(lib, O, device=False):
    """the same six through both front-end twins: the fingerprint and the names of the IR built through the C ABI, and its rows"""
    coords, topo = blob12k(O, 4)
    s = sets_of(topo)
    ir_abi = count_ir(lib, blob_props(s))
    ir_py, info = script.compile_script(BLOB_SCRIPT, topo, lib=lib, **BITS)
    ir_c = script.compile_script_native(BLOB_SCRIPT, topo, lib=lib, **BITS)
    assert ir_abi.fingerprint() == ir_py.fingerprint() == ir_c.fingerprint()
    assert ir_abi.property_names() == ir_py.property_names() == ir_c.property_names() == list(CUBIC_POPS)
    assert [len(info[k]["terms"]) for k in CUBIC_POPS] == [2, 2, 2, 2, 1, 4]
    assert [info[k]["truth"] for k in CUBIC_POPS] == [X.AND2, X.A_NOT_B, X.XOR2, X.OR2, X.NOT1, FOUR]
    want = blob_reference(O, "cubic")
    ev = evaluate(lib, ir_c, coords, 50.0, device=device)
    for k in want:
        assert np.array_equal(rows(ev, k)[:, 0], want[k]), k


def test_both_twins_on_the_blob_system(emu_lib, oracle):
    twins_on_the_blob(emu_lib, oracle)


# ---- 3. kernel edges ---------------------------------------------------------------------------------------------------------------------

SIZES = (1, 63, 64, 65, 255, 256, 257, 513)


def kernel_edges(lib, O, device=False):
    """lists cut from the blob system's water oxygens so that, in frame 0, the members of `A and not B` stand in the first and the last
    lane of a wave and of a block and nowhere else; a list whose first wave term 0 decides whole, next to a wave with one live lane; every
    size at which a block or a wave fills up; one term negated and four terms; batches of 1 and 3 frames; host and device trajectories"""
    import cases
    coords, topo = blob12k(O, 3)
    s = sets_of(topo)
    pool, _ = blob_exprs(s)
    A, B = pool[0], pool[1]
    bx = X.as_box(50.0)
    idx0 = X.outcomes(coords[0], bx, s["wo"], [A, B])
    ins, outs, h0_off = s["wo"][idx0 == 1], s["wo"][idx0 != 1], s["wo"][(idx0 & 1) == 0]
    h0_on = s["wo"][(idx0 & 1) == 1]
    planted_at = [0, 63, 64, 127, 255, 256, 511, 512]
    planted = outs[:513].copy()
    planted[planted_at] = ins[:len(planted_at)]
    decided = np.concatenate([h0_off[:64], h0_off[64:127], h0_on[:1], h0_off[127:140]]).astype(np.int32)      # wave 1: one live lane, its last
    props = [("planted", planted, [A, B], X.A_NOT_B), ("decided", decided, [A, B], X.AND2), ("decided_or", decided, [A, B], X.OR2)]
    for n in SIZES:
        props.append((f"not{n}", s["wo"][:n], [pool[2]], X.NOT1))
        props.append((f"four{n}", s["wo"][100:100 + n], [pool[3], A, B, pool[4]], FOUR))
    want = {name: X.counts(coords, bx, t, terms, tr) for name, t, terms, tr in props}
    assert want["planted"][0] == len(planted_at) and want["decided"][0] <= 1 and want["decided_or"][0] >= 1
    assert any(0 < want[f"not{n}"][0] < n for n in SIZES) and any(want[f"four{n}"].any() for n in SIZES)
    ir = count_ir(lib, props)
    cell = V.make_unitcell(50.0)
    sysm = V.MolSystem(coords.shape[2], unitcell=cell)
    devices = [False, True] if (device or lib.vmd_device_count() > 0) else [False]
    for dev in devices:
        for bf in (0, 1, 3):
            for skip in (1, 0):
                with options(lib, batch_frames=bf, shell_expr_skip=skip):
                    ev = evaluate(lib, ir, coords, 50.0, device=dev)
                for name in want:
                    assert np.array_equal(rows(ev, name)[:, 0], want[name]), (dev, bf, skip, name, rows(ev, name)[:, 0], want[name])
        # the members themselves, by atom: exactly the planted ones
        traj = cases.make_traj(lib, coords, cell, dev)
        m = ev.shell_mask("planted", sysm, traj, 0)
        assert np.array_equal(np.nonzero(m)[0], np.sort(planted[planted_at]))
        for name, t, terms, tr in props[:3] + props[-2:]:
            for f in (0, 2):
                assert np.array_equal(ev.shell_mask(name, sysm, traj, f), X.atom_mask(coords[f], bx, t, terms, tr, coords.shape[2])), (name, f)


def test_kernel_edges_on_the_emulator(emu_lib, oracle):
    kernel_edges(emu_lib, oracle)


# ---- 4. identities that need no yardstick ---------------------------------------------------------------------------------------------------

IDENTITY_SCRIPT = ("s1 = resname(\"ALA\")[2:8];"
                   "n_ab = count(water and element('O') and within(3.5, atom(1:100)) and within(3.5, atom(101:200)));"
                   "n_anb = count(water and element('O') and within(3.5, atom(1:100)) and not within(3.5, atom(101:200)));"
                   "n_a = count(water and element('O') and within(3.5, atom(1:100)));"
                   "v_ab = sdf(s1, water and element('O') and within(3.5, atom(1:100)) and within(3.5, atom(101:200)), 10.0);"
                   "v_anb = sdf(s1, water and element('O') and within(3.5, atom(1:100)) and not within(3.5, atom(101:200)), 10.0);"
                   "v_a = sdf(s1, water and element('O') and within(3.5, atom(1:100)), 10.0);")


ONE_TERM_SCRIPT = ("s1 = resname(\"ALA\")[2:8]; n_a = count(water and element('O') and within(3.5, atom(1:100)));"
                   "v_a = sdf(s1, water and element('O') and within(3.5, atom(1:100)), 10.0);")


def identities(lib, O, device=False, F=6):
    import cases
    coords, topo = TG.blob_system(O, n_atoms=3000, n_blob=200, F=F)
    mass = np.asarray(topo.mass, np.float32)
    ir, info = script.compile_script(IDENTITY_SCRIPT, topo, lib=lib, **BITS)
    # n_a and v_a ARE today's one-term properties: the script without the new bit gives them the same descriptors
    old = script.compile_script(ONE_TERM_SCRIPT, topo, lib=lib, within=True, shell_sdf=True)[0]
    new = script.compile_script(ONE_TERM_SCRIPT, topo, lib=lib, **BITS)[0]
    assert old.fingerprint() == new.fingerprint() and old.property_names() == ["n_a", "v_a"]
    assert info["n_a"]["kind"] == "within_count" and info["n_ab"]["kind"] == "within_count_expr" and "target_shell" in info["v_a"]
    ev = evaluate(lib, ir, coords, 30.0, device=device, mass=mass)
    n_ab, n_anb, n_a = (rows(ev, k)[:, 0] for k in ("n_ab", "n_anb", "n_a"))
    assert np.array_equal(n_ab + n_anb, n_a) and n_ab.sum() > 0 and n_anb.sum() > 0 and len(set(n_a.tolist())) > 1
    assert np.array_equal(vol(ev, "v_ab") + vol(ev, "v_anb"), vol(ev, "v_a")) and vol(ev, "v_ab").sum() > 0 and vol(ev, "v_anb").sum() > 0
    cell = V.make_unitcell(30.0)
    sysm, traj = V.MolSystem(coords.shape[2], mass=mass, unitcell=cell), cases.make_traj(lib, coords, cell, device)
    bx = X.as_box(30.0)
    for name, cnt in (("n_ab", n_ab), ("n_anb", n_anb)):
        i = info[name]
        terms = [(t["ref"], t["rmin"], t["rmax"]) for t in i["terms"]]
        for f in range(F):
            m = ev.shell_mask(name, sysm, traj, f)
            assert int(m.sum()) == int(cnt[f])                                              # the population is the count row of that frame
            assert np.array_equal(m, X.atom_mask(coords[f], bx, i["target"], terms, i["truth"], coords.shape[2])), (name, f)
            assert np.array_equal(m, ev.shell_mask("v" + name[1:], sysm, traj, f))         # the sdf over the same expression shares it
    for which, name in ((0, "n_ab"), (0, "v_anb")):
        with pytest.raises(V.VmdError, match="not a within"):
            ev.shell_mask(name, sysm, traj, 0, which=which)


def test_identities(emu_lib, oracle):
    identities(emu_lib, oracle)


def sdf_against_the_yardstick(lib, O, device=False):
    """the sdf form against shell_sdf_ref's loop with the membership supplied by the restatement; D-SDF-EXCL and an empty frame included"""
    coords, topo, s, st, mass = TS.blob_case(O, 3)
    pool, _ = blob_exprs(s)
    T = np.concatenate([s["blob"][:60], s["wo"]]).astype(np.int32)              # names members of the structures
    terms = [pool[0], pool[1]]
    want, pops = X.sdf(O, coords, 50.0, st, mass, T, terms, X.A_NOT_B, 10.0)
    static, _ = TS.S.shell_sdf(O, coords, 50.0, st, mass, (T, None), 10.0)
    caps(want, pops, static, T.size)
    for opt in (dict(shell_brute_below=0), dict(force_brute=1)):
        ir = V.ScriptIR(lib)
        ir.add_sdf_shell_expr("v", st, T, 10.0, terms, X.A_NOT_B)
        ir.add_sdf_shell_expr("none", st, T, 10.0, terms, 0)                     # a constant table: empty in every frame
        with options(lib, **opt):
            ev = evaluate(lib, ir, coords, 50.0, device=device, mass=mass)
        TS.check(ev, "v", want, 10.0)
        assert not vol(ev, "none").any() and ev.frame_mask().all()


def test_sdf_against_the_yardstick(emu_lib, oracle):
    sdf_against_the_yardstick(emu_lib, oracle)


# ---- 5. overflow, call patterns, co-evaluation, multi-rank -------------------------------------------------------------------------------------

def overflow_case(lib, O, device=False):
    """the device of test_within.overflow_case: the middle frames pile every oxygen into one pencil, a bucket of the cell build of a
    reference set overflows, the batch - builds, term passes, finish - is repeated and every frame is counted once"""
    import cases
    n, box, F = 3000, 60.0, 12
    coords = cases.water_box(O, 5, n, box, F)
    o, h = cases.oxygen(n), cases.hydrogen(n)
    rng = np.random.default_rng(3)
    for f in (5, 6, 7):
        coords[f][:, o] = rng.uniform(1.0, 11.0, (3, o.size)).astype(np.float32)
    st = np.stack([np.arange(3 * k, 3 * k + 3) for k in (10, 400)]).astype(np.int32)
    mass = np.tile(np.float32([15.999, 1.008, 1.008]), n // 3)
    terms = [(h[::2], 0.0, 3.0), (o, 1.0, 4.0)]
    props = [("n", o, terms, X.AND2), ("m", o, terms, X.XOR2)]          # (a and not b has no member in the piled frames: every oxygen has a neighbour)
    want = {nm: X.counts(coords, box, t, tm, tr) for nm, t, tm, tr in props}
    for w in want.values():
        varied(w, o.size)
    vwant, pops = X.sdf(O, coords, box, st, mass, o, terms, X.AND2, 12.0)
    assert np.array_equal(pops.astype(np.float32), want["n"]) and vwant.sum() > 0
    with options(lib, cells_small=0, cells_cap_sample=2, shell_brute_below=0):
        for bf, defer in ((0, 1), (4, 1), (4, 0)):
            with options(lib, batch_frames=bf, defer_sync=defer):
                ir = count_ir(lib, props)
                ir.add_sdf_shell_expr("v", st, o, 12.0, terms, X.AND2)
                ev = evaluate(lib, ir, coords, box, device=device, mass=mass)
                assert ev.cell_build_stats()[0] >= 1, (bf, defer)
                for nm in want:
                    assert np.array_equal(rows(ev, nm)[:, 0], want[nm]), (bf, defer, nm)
                TS.check(ev, "v", vwant, 12.0)


def test_a_bucket_overflow_repeats_the_batch_and_counts_once(emu_lib, oracle):
    overflow_case(emu_lib, oracle)


CALL_SCRIPT = ("s1 = resname(\"ALA\")[2:8];"
               "nb = count(water and element('O') and within(3.5, atom(1:100)) and within(3.5, atom(101:200)));"
               "far = count(water and element('O') and not within(5.0, not water));"
               "vn = sdf(s1, water and element('O') and within(6.0, not water) and not within(3.5, not water), 10.0);"
               "one = count(water and element('O') and within(3.5, atom(1:100)));"
               "g = rdf(element('O'), element('O'), 3.5); d = distance(10, 30);")
RAGGED = [(0, 7), (7, 8), (8, 21), (21, 30)]


def call_patterns(lib, O, device=False):
    coords, topo = TG.blob_system(O, n_atoms=3000, n_blob=200, F=30)
    mass = np.asarray(topo.mass, np.float32)
    ir, info = script.compile_script(CALL_SCRIPT, topo, lib=lib, **BITS)
    run = lambda **kw: evaluate(lib, ir, coords, 30.0, device=device, mass=mass, **kw)
    with options(lib, shell_brute_below=0):           # the walk: the path with state between batches
        one_call = run()
        got = {"grain 1": run(pooled=(16, 1)), "grain 4": run(pooled=(4, 4)), "ragged": run(ranges=RAGGED), "late first": run(ranges=RAGGED[::-1])}
        for bf in (3, 16):
            with options(lib, batch_frames=bf):
                got[f"batch_frames {bf}"] = run()
        with options(lib, readahead=0):
            got["no read-ahead"] = run(pooled=(8, 1))
    got["the rule's own choice"] = run()
    with options(lib, force_brute=1):
        got["all pairs"] = run()
    with options(lib, shell_expr_skip=0):
        got["every lane live"] = run()
    for name in ("nb", "far"):
        i = info[name]
        want = X.counts(coords, 30.0, i["target"], [(t["ref"], t["rmin"], t["rmax"]) for t in i["terms"]], i["truth"])
        assert want.any() and len(set(want.tolist())) > 1
        assert np.array_equal(rows(one_call, name)[:, 0], want), name
    assert vol(one_call, "vn").sum() > 0
    for what, ev in got.items():
        for name in ("nb", "far", "one", "d"):
            assert bits_equal(rows(ev, name), rows(one_call, name)), (what, name)
        assert np.array_equal(vol(ev, "vn"), vol(one_call, "vn")), what
        assert np.array_equal(ev.property_data("g").counts, one_call.property_data("g").counts), what


def test_call_patterns(emu_lib, oracle):
    call_patterns(emu_lib, oracle)


STATIC_SCRIPT = ("s1 = resname(\"ALA\")[2:8]; goo = rdf(element('O'), element('O'), 8.0); v = sdf(s1, element('H'), 10.0);"
                 "nw = count(water and element('O') and within(3.5, atom(1:100))); d = distance(10, 30);"
                 "vs = sdf(s1, water and element('O') and within(3.5, atom(101:200)), 10.0);")
EXPR_LINES = ("nb = count(water and element('O') and within(3.5, atom(1:100)) and within(3.5, atom(101:200)));"
              "vx = sdf(s1, water and element('O') and within(3.5, atom(101:200)) and not within(3.5, atom(1:100)), 10.0);")


def coevaluation(lib, O, device=False):
    """static properties and the one-term shells that share R with the expressions are what they are without the expression lines"""
    coords, topo = TG.blob_system(O, n_atoms=3000, n_blob=200, F=4)
    mass = np.asarray(topo.mass, np.float32)
    ev0 = evaluate(lib, script.compile_script(STATIC_SCRIPT, topo, lib=lib, within=True, shell_sdf=True)[0], coords, 30.0, device=device, mass=mass)
    ir1, info = script.compile_script(STATIC_SCRIPT + EXPR_LINES, topo, lib=lib, **BITS)
    with options(lib, shell_brute_below=0):
        ev1 = evaluate(lib, ir1, coords, 30.0, device=device, mass=mass)
    for name in ("goo", "v", "nw", "d", "vs"):
        a, b = ev0.property_data(name), ev1.property_data(name)
        assert bits_equal(a.values, b.values) and np.asarray(a.values).any(), name
        if a.counts is not None:
            assert np.array_equal(a.counts, b.counts), name
    i = info["nb"]
    want = X.counts(coords, 30.0, i["target"], [(t["ref"], t["rmin"], t["rmax"]) for t in i["terms"]], i["truth"])
    assert np.array_equal(rows(ev1, "nb")[:, 0], want) and want.any()
    assert (vol(ev1, "vx") <= vol(ev1, "vs")).all() and vol(ev1, "vx").sum() > 0


def test_static_properties_are_unchanged_by_expression_lines(emu_lib, oracle):
    coevaluation(emu_lib, oracle)


MERGE_SCRIPT = ("s1 = resname(\"ALA\")[2:8]; nb = count(water and element('O') and within(3.5, atom(1:100)) and not within(3.5, atom(101:200)));"
                "vn = sdf(s1, water and element('O') and within(6.0, not water) and not within(3.5, not water), 10.0); d = distance(10, 30);")


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
    ir = script.compile_script(MERGE_SCRIPT, topo, lib=lib, **BITS)[0]
    F = coords.shape[0]
    ev = V.ScriptEval(F, ir)
    beg, end = shard_frames(F, rank, world)
    cell = V.make_unitcell(30.0)
    assert ev.frame_range(V.MolSystem(coords.shape[2], unitcell=cell), V.HostTrajectory(coords, cell), beg, end)
    reduce_eval(ev)
    assert ev.frame_mask().all()
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), nb=ev.property_data("nb").values, d=ev.property_data("d").values,
             vn=np.asarray(ev.property_data("vn").counts))
    dist.destroy_process_group()


def test_two_rank_merge_equals_the_single_evaluation(emu_lib, oracle, tmp_path):
    import torch.multiprocessing as mp
    port = 45500 + (os.getpid() % 2000)
    mp.spawn(_merge_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    coords, topo = TG.blob_system(oracle, n_atoms=3000, F=7)
    ir = script.compile_script(MERGE_SCRIPT, topo, lib=emu_lib, **BITS)[0]
    one_rank = evaluate(emu_lib, ir, coords, 30.0)
    assert rows(one_rank, "nb").any() and vol(one_rank, "vn").sum() > 0
    for r in range(2):
        z = np.load(tmp_path / f"rank{r}.npz")
        for n in ("nb", "d"):
            assert bits_equal(z[n].reshape(7, -1), rows(one_rank, n)), n
        assert np.array_equal(z["vn"], vol(one_rank, "vn"))


# ---- 6. front-end --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def topo():
    return synth.water_box_topology(200 + 933 * 3, n_blob=200)


OLD_BITS = dict(angles=True, shape=True, rmsd=True, within=True, shell_rdf=True, shell_sdf=True)
ALL_BITS = dict(OLD_BITS, shell_expr=True)
A_, B_ = "within(3.5, atom(1:100))", "within(3.5, atom(101:200))"
AND3 = X.table(lambda a, b, c: a and b and c, 3)

# statement, |T|, [(|R|, rmin, rmax)], truth
ACCEPTED = [
    (f"n = count(water and {A_} and {B_});", 2799, [(100, 0.0, 3.5), (100, 0.0, 3.5)], X.AND2),
    (f"n = count(element('O') and not {A_});", 953, [(100, 0.0, 3.5)], X.NOT1),
    (f"n = count(not {A_});", 2999, [(100, 0.0, 3.5)], X.NOT1),
    (f"n = count(({A_} or {B_}) and water and element('O'));", 933, [(100, 0.0, 3.5), (100, 0.0, 3.5)], X.OR2),
    (f"n = count(water and not ({A_} and not (within(2.8:3.2, element('N')))));", 2799, [(100, 0.0, 3.5), (20, 2.8, 3.2)],
     X.table(lambda a, b: not (a and not b), 2)),
    (f"n = count(water and {A_} and {B_} and {A_});", 2799, [(100, 0.0, 3.5), (100, 0.0, 3.5)], X.AND2),            # a repeated term is one term
    (f"n = count(water and {B_} and not {B_});", 2799, [(100, 0.0, 3.5)], 0),                                     # a constant table
    (f"n = count(water and ({A_} or not {A_}) and {B_});", 2799, [(100, 0.0, 3.5), (100, 0.0, 3.5)], 0b1100),      # a table that ignores a term
    (f"n = count(water and {A_} and {B_} and within(5.0, protein));", 2799, [(100, 0.0, 3.5), (100, 0.0, 3.5), (200, 0.0, 5.0)], AND3),
    (f"n = count({A_} and {B_} and within(5.0, protein) and not within(1.0:2.0, water));", 2999,
     [(100, 0.0, 3.5), (100, 0.0, 3.5), (200, 0.0, 5.0), (2799, 1.0, 2.0)], X.table(lambda a, b, c, d: a and b and c and not d, 4)),
    (f"s1 = resname(\"ALA\")[2:8]; n = sdf(s1, element('O') and {A_} and not {B_}, 10.0);", 953, [(100, 0.0, 3.5), (100, 0.0, 3.5)], X.A_NOT_B),
]

SKIPPED = [
    (f"n = count(water and {A_} and {B_} and within(5.0, protein) and within(1.0:2.0, water) and within(4.0, water));",
     "n: more than four distinct within() terms"),
    (f"n = count(water and ({A_} or element('O')));", "n: a static selection inside a parenthesised dynamic factor"),
    (f"n = count(water and not ({A_} and water));", "n: a static selection inside a parenthesised dynamic factor"),
    ("n = count(water and within(3, within(4, protein)));", "n: within() nested in a within() argument"),
    (f"n = count(water or {A_});", "n: a dynamic factor under a top-level or with a static selection"),
    (f"n = count(water and {A_} or element('O'));", "n: a dynamic factor under a top-level or with a static selection"),
    (f"s1 = resname(\"ALA\")[2:8]; n = sdf(s1, element('O') or {A_}, 10.0);", "n: a dynamic factor under a top-level or with a static selection"),
    (f"n = count(resname(\"XYZ\") and {A_} and {B_});", "n: empty selection"),
    (f"n = count(water and {A_} and not within(3, resname(\"XYZ\")));", "n: empty selection"),
    (f"n = count(water and {A_} and not within(0, protein));", "within needs a radius > 0"),
    (f"n = count(water and {A_} and within(5:3, protein));", "within range needs 0 <= a < b"),
    ("n = count(water);", "count of a static selection is a constant (left to the fallback)"),
    (f"n = count(water and {A_} and {B_}) in resname(\"ALA\");", "count(...) in <contexts> is outside the subset"),
    # unchanged: rdf arguments, the distance family and the sdf structures keep their messages
    (f"n = rdf(water and {A_} and {B_}, water, 5.0);", "an rdf argument takes exactly one within() factor, found 2"),
    (f"n = rdf(water and not {A_}, water, 5.0);", "within() must be a factor of the top-level AND"),
    (f"n = distance({A_} and {B_}, water);", "unsupported function 'within'"),
    (f"n = sdf({A_} and {B_}, water, 5.0);", "within() in the structures argument of sdf() is not supported"),
]


@pytest.mark.parametrize("stmt,nt,terms,truth", ACCEPTED)
def test_accepted_forms(host_lib, topo, stmt, nt, terms, truth):
    ir_c = script.compile_script_native(stmt, topo, lib=host_lib, **ALL_BITS)
    ir_py, info = script.compile_script(stmt, topo, lib=host_lib, **ALL_BITS)
    assert ir_c.property_names() == ir_py.property_names() == ["n"] and ir_c.fingerprint() == ir_py.fingerprint()
    i = info["n"]
    assert len(i["target"]) == nt and i["truth"] == truth
    assert [(len(t["ref"]), t["rmin"], t["rmax"]) for t in i["terms"]] == [(n, float(np.float32(a)), float(np.float32(b))) for n, a, b in terms]
    # the C ABI with the same lists is the same IR
    q = V.ScriptIR(host_lib)
    tl = [(t["ref"], t["rmin"], t["rmax"]) for t in i["terms"]]
    if i["kind"] == "sdf":
        q.add_sdf_shell_expr("n", i["structures"], i["target"], i["cutoff"], tl, truth)
        assert ir_c.geometry_atoms("n").size == 0
        static = V.ScriptIR(host_lib); static.add_sdf("n", i["structures"], i["target"], i["cutoff"])
        assert int(host_lib.vmd_ir_work_per_frame(ir_c.h)) == int(host_lib.vmd_ir_work_per_frame(static.h)) + nt + sum(n for n, _, _ in terms)
    else:
        q.add_within_count_expr("n", i["target"], tl, truth)
        assert list(ir_c.geometry_atoms("n")) == [a for t in i["terms"] for a in t["ref"]] + list(i["target"])
        assert int(host_lib.vmd_ir_work_per_frame(ir_c.h)) == nt + sum(n for n, _, _ in terms)
    assert q.fingerprint() == ir_c.fingerprint()


@pytest.mark.parametrize("stmt,reason", SKIPPED)
def test_skipped_forms(host_lib, topo, stmt, reason):
    text = "d = distance(1, 2);\n" + stmt + "\ne = distance(3, 4);"
    for compiler in (script.compile_script_native, script.compile_script):
        with pytest.raises((script.ScriptError, V.VmdError)) as err:
            compiler(text, topo, lib=host_lib, **ALL_BITS)
        assert reason in str(err.value)
    ir_c, rep_c = script.compile_script_native(text, topo, lib=host_lib, partial=True, **ALL_BITS)
    ir_py, _, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, **ALL_BITS)
    assert ir_c.property_names() == ir_py.property_names() == ["d", "e"] and ir_c.fingerprint() == ir_py.fingerprint()
    assert rep_c == rep_py and len(rep_c["skipped"]) == 1
    k = rep_c["skipped"][0]
    assert k["names"] == "n" and reason in k["reason"] and text[k["beg"]:k["end"]].endswith(stmt.split("; ")[-1][:-1])
    assert "distance(3, 4)" not in rep_c["fallback_source"]


def test_one_positive_term_is_the_one_term_property(host_lib, topo):
    """under the new bit, count(T and within) and sdf(s, T and within) - plain, parenthesised, doubly negated, repeated - compile to the
    descriptors vmd_ir_add_within_count / vmd_ir_add_sdf_shell build, and so do the new entry points with one term and truth 0b10"""
    base_c = f"n = count(water and {A_});"
    base_s = f"s1 = resname(\"ALA\")[2:8]; n = sdf(s1, element('O') and {A_}, 10.0);"
    for base, variants in ((base_c, [f"n = count(water and ({A_}));", f"n = count(water and not not {A_});", f"n = count({A_} and water and {A_});",
                                     f"n = count(water and ({A_} or {A_}));"]),
                           (base_s, [f"s1 = resname(\"ALA\")[2:8]; n = sdf(s1, element('O') and ({A_}), 10.0);",
                                     f"s1 = resname(\"ALA\")[2:8]; n = sdf(s1, not not {A_} and element('O'), 10.0);"])):
        want = script.compile_script_native(base, topo, lib=host_lib, **OLD_BITS).fingerprint()
        for text in [base] + variants:
            for compiler in (script.compile_script_native, script.compile_script):
                got = compiler(text, topo, lib=host_lib, **ALL_BITS)
                assert (got[0] if isinstance(got, tuple) else got).fingerprint() == want, text
    t, r = np.arange(5, dtype=np.int32), np.arange(5, 9, dtype=np.int32)
    a = V.ScriptIR(host_lib); a.add_within_count("n", t, r, 0.5, 3.0)
    b = V.ScriptIR(host_lib); b.add_within_count_expr("n", t, [(r, 0.5, 3.0)], 0b10)
    c = V.ScriptIR(host_lib); c.add_within_count_expr("n", t, [(r, 0.5, 3.0)], 0b01)
    assert a.fingerprint() == b.fingerprint() != c.fingerprint()
    st = np.arange(10, 16, dtype=np.int32).reshape(2, 3)
    a = V.ScriptIR(host_lib); a.add_sdf_shell("n", st, t, 5.0, target_shell=(r, 0.5, 3.0))
    b = V.ScriptIR(host_lib); b.add_sdf_shell_expr("n", st, t, 5.0, [(r, 0.5, 3.0)], 0b10)
    c = V.ScriptIR(host_lib); c.add_sdf_shell_expr("n", st, t, 5.0, [(r, 0.5, 3.0)], 0b01)
    assert a.fingerprint() == b.fingerprint() != c.fingerprint()


ISSUE_LINES = [("nb = count(element('O') and within(3.5, atom(1:100)) and within(3.5, protein));", "count takes exactly one within() factor, found 2"),
               ("bulk = count(element('O') and not within(5.0, protein));", "within() must be a factor of the top-level AND"),
               ("v = sdf(s1, element('O') and within(3.5, s1) and not within(3.5, atom(1:100)), 10.0);", "an sdf argument takes exactly one within() factor, found 2"),
               ("ne = count(element('O') and (within(3.5, atom(1:100)) or within(2.8:3.2, element('N'))));", "count takes exactly one within() factor, found 2")]


def test_without_the_bit_nothing_changes(host_lib, topo):
    import test_rmsd
    assert test_rmsd._old_ir(host_lib).fingerprint() == test_rmsd.PARENT_FINGERPRINT          # the literal the parent's suite holds
    text = "s1 = resname(\"ALA\")[2:8];\n" + "\n".join(ln for ln, _ in ISSUE_LINES) + "\nd = distance(1, 2);"
    res = [script.compile_script_native(text, topo, lib=host_lib, partial=True, **OLD_BITS),
           script.compile_script_native(text, topo, lib=host_lib, partial=True, shell_expr=False, **OLD_BITS),
           script.compile_script(text, topo, lib=host_lib, partial=True, shell_expr=False, **OLD_BITS)[::2]]
    for ir, rep in res:
        assert ir.property_names() == ["d"] and ir.fingerprint() == res[0][0].fingerprint() and rep == res[0][1]
        assert [k["names"] for k in rep["skipped"]] == ["nb", "bulk", "v", "ne"]
        for k, (_, reason) in zip(rep["skipped"], ISSUE_LINES):
            assert reason in k["reason"]                                                    # the words the parent commit gives
    # with the bit, the four lines compile on both twins, to the same IR
    ir_c, rep_c = script.compile_script_native(text, topo, lib=host_lib, partial=True, **ALL_BITS)
    ir_py, _, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, **ALL_BITS)
    assert ir_c.property_names() == ir_py.property_names() == ["nb", "bulk", "v", "ne", "d"] and rep_c == rep_py and rep_c["skipped"] == []
    assert ir_c.fingerprint() == ir_py.fingerprint()
    # the bit alone enables nothing: count() needs the within bit, the sdf target the shell_sdf bit
    for compiler in (script.compile_script_native, script.compile_script):
        with pytest.raises(script.ScriptError, match="unsupported function 'count'"):
            compiler(ISSUE_LINES[1][0], topo, lib=host_lib, shell_expr=True)
        with pytest.raises(script.ScriptError, match="unsupported function 'within'"):
            compiler("s1 = resname(\"ALA\")[2:8];" + ISSUE_LINES[2][0], topo, lib=host_lib, within=True, shell_expr=True)
    # scripts without the new forms keep their fingerprints and reports whatever the new bit says
    for text0 in (TG.VIAMD_DEFAULT_SCRIPT + TW.NW_LINE + TS.GS_LINE, "x = within(3, all); g = rdf(all, within(3, all), 5.0); d = distance(1, 2);"):
        res = [script.compile_script_native(text0, topo, lib=host_lib, partial=True, shell_expr=w, **OLD_BITS) for w in (False, True)]
        res.append(script.compile_script(text0, topo, lib=host_lib, partial=True, **ALL_BITS)[::2])
        assert len({r[0].fingerprint() for r in res}) == 1 and res[0][1] == res[1][1] == res[2][1], text0


def test_ir_validation_errors(host_lib):
    lib = host_lib
    for sym in ("vmd_ir_add_within_count_expr", "vmd_ir_add_sdf_shell_expr", "vmd_hip_within_atoms_expr", "vmd_hip_within_brute_expr",
                "vmd_hip_shell_expr_finish"):
        assert hasattr(lib, sym), sym
    assert script.FEATURE_SHELL_EXPR == 64 and L.SHELL_EXPR_MAX_TERMS == 4
    assert lib.vmd_set_option(b"shell_expr_skip", 1) == 1                                   # the default
    ir = V.ScriptIR(lib)
    ok = ([1], 0.0, 3.0)
    st = np.arange(10, 16, dtype=np.int32).reshape(2, 3)
    for add in (lambda *a: ir.add_within_count_expr("n", [0, 2], *a), lambda *a: ir.add_sdf_shell_expr("n", st, [0, 2], 5.0, *a)):
        for terms, truth, msg in (([], 0, "1 to 4 terms"), ([ok] * 5, 0, "1 to 4 terms"), ([ok], 0b100, "truth table has bits above"),
                                  ([ok, ok], 1 << 16, "truth table has bits above"), ([([], 0.0, 3.0)], 2, "reference set is empty"),
                                  ([ok, ([1, -1], 0.0, 3.0)], 2, "negative"), ([ok, ([1], 3.0, 3.0)], 2, "0 <= rmin < rmax"),
                                  ([([1], 0.0, float("inf"))], 1, "finite"), ([ok, ([1], float("nan"), 3.0)], 1, "finite")):
            with pytest.raises(V.VmdError, match=msg):
                add(terms, truth)
    with pytest.raises(V.VmdError, match="target set is empty"):
        ir.add_within_count_expr("n", [], [ok], 1)
    with pytest.raises(V.VmdError, match="name is empty"):
        ir.add_within_count_expr("", [0], [ok], 1)
    p = lambda x: x.ctypes.data_as(L.c_int32_p)
    a = np.array([0, 1], np.int32)
    assert not lib.vmd_ir_add_within_count_expr(ir.h, b"n", p(a), 2, None) and "shell expression is NULL" in lib.last_error()
    assert not lib.vmd_ir_add_sdf_shell_expr(ir.h, b"n", p(st.ravel()), 2, 3, p(a), 2, None, 5.0) and "shell expression is NULL" in lib.last_error()
    assert ir.property_count() == 0
    ir.add_distance("d", [0], [1])
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_within_count_expr("d", [0], [ok], 1)
    ir.add_within_count_expr("n", [0, 5, 7], [([1, 5], 0.5, 3.0), ([2], 0.0, 1.0)], 0b0110)
    ir.add_within_count_expr("c0", [0], [ok, ok], 0)                                        # constant tables are accepted
    ir.add_within_count_expr("c1", [0], [ok], 0b11)
    assert ir.property_names() == ["d", "n", "c0", "c1"] and ir.property_flags("n") == L.FLAG_TEMPORAL
    assert list(ir.geometry_atoms("n")) == [1, 5, 2, 0, 5, 7] and ir.geometry_atoms("n", 1).size == 0
    assert int(lib.vmd_ir_work_per_frame(ir.h)) == 1 + (3 + 3) + (1 + 2) + (1 + 1)

    def fp(*args):
        q = V.ScriptIR(lib)
        q.add_within_count_expr(*args)
        return q.fingerprint()
    base = ("n", [0, 1, 2], [([3, 4], 0.0, 3.0), ([5], 0.0, 3.0)], X.AND2)
    variants = [base, ("m",) + base[1:], base[:3] + (X.OR2,), ("n", [0, 1], base[2], X.AND2), ("n", [0, 1, 2], [([3], 0.0, 3.0), ([4, 5], 0.0, 3.0)], X.AND2),
                ("n", [0, 1, 2], [([3, 4], 0.0, 3.0), ([5], 0.5, 3.0)], X.AND2), ("n", [0, 1, 2], [([3, 4], 0.0, 3.0), ([5], 0.0, 3.5)], X.AND2),
                ("n", [0, 1, 2], [([5], 0.0, 3.0), ([3, 4], 0.0, 3.0)], X.AND2), ("n", [0, 1, 2], [([3, 4], 0.0, 3.0)], X.NOT1)]
    assert len({fp(*v) for v in variants}) == len(variants)
    ir2 = V.ScriptIR(lib)
    ir2.add_within_count_expr("n", [0, 1], [([1], 0.0, 3.0), ([99], 0.0, 3.0)], X.AND2)
    if lib.vmd_device_count() > 0:
        with pytest.raises(V.VmdError, match="references atom 99"):
            TG.evaluate(lib, ir2, np.zeros((1, 3, 10), np.float32), 10.0)


def test_the_live_words_of_the_term_passes(emu_lib):
    """constant tables and a table that ignores a term launch no pass for what cannot matter; results are the table's"""
    pts = np.array([(10, 10, 10), (14, 10, 10), (12, 10, 10), (30, 30, 30)], np.float32)
    xyz = np.ascontiguousarray(pts.T[None])
    terms = [([0], 0.0, 3.0), ([1], 0.0, 3.0)]
    for truth, passes, want in ((0, 0, 0), (0xF, 0, 2), (0b1100, 1, 1), (0b1010, 1, 1), (X.AND2, 2, 1)):
        got, n = profiled(emu_lib, lambda: count_rows(emu_lib, [("n", [2, 3], terms, truth)], xyz, 50.0))
        assert got["n"].tolist() == [want] and n["shell_expr_brute"] == passes and n["shell_expr_finish"] == 1, (truth, got, n)
        got, n = profiled(emu_lib, lambda: count_rows(emu_lib, [("n", [2, 3], terms, truth)], xyz, 50.0), shell_expr_skip=0)
        assert got["n"].tolist() == [want] and n["shell_expr_brute"] == 2, (truth, got, n)


# ---- 7. VIAMD's default script plus a bridging count and a second-shell sdf through the shim ---------------------------------------------------

def build_shim_shell_expr():
    """tests/native/shim_default_script_shell_expr.cpp linked against the product library"""
    return native_host.build_shim("shim_default_script_shell_expr")


def test_shim_default_script_with_the_expression_lines_on_the_emulator(emu_lib, tmp_path):
    import conftest
    exe = native_host.build_shim("shim_default_script_shell_expr", conftest.build_emu(), tmp_path / "shim_shell_expr_emu")
    native_host.run_ok([exe, "8"], "OK frames=8 properties=9 expr=gpu fallback_frame_range_calls=0")
    out = native_host.run_ok([exe, "8", "nobit"], "OK frames=8 properties=9 expr=fallback")
    assert "fallback_frame_range_calls=0" not in out.stdout, out.stdout
