"""count(T and within(r, R)) on the emulator build and in the host-only entry points: known answers, exactness at the
interval ends, both kernels against the numpy restatement (tests/within_ref.py), script-level parity, the cross-check against rdf(),
call patterns, a pencil-bucket overflow, the row offsets of a script with its temporal properties in an unusual order, multi-rank
merges, export, the opt-in front-end (C++ and Python twin), ABI validation and VIAMD's default script plus a hydration-number line
through the shim.  Counts are integers: every comparison is `==`."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import native_host

import viamd_amd as V
from viamd_amd import _lib as L
from viamd_amd import script, synth

import within_ref as W
import test_geometry as TG
from test_geometry import bits_equal, rows
from geometry_ref import Box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIAMD_DEFAULT_SCRIPT = TG.VIAMD_DEFAULT_SCRIPT
NW_LINE = "\nnw = count(element('O') and within(3.5, resname(\"ALA\")));"
TILT = (12.0, -8.0, 10.0)


class options:
    """vmd_set_option for the length of a with block"""

    def __init__(self, lib, **kw):
        self.lib, self.kw, self.old = lib, kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = self.lib.vmd_set_option(k.encode(), int(v))

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.lib.vmd_set_option(k.encode(), v)


def launches(lib, key):
    nb = C.c_uint64(0)
    lib.vmd_profile_ms(key.encode(), C.byref(nb))
    return int(nb.value)


def evaluate(lib, ir, coords, box, tilt=(0.0, 0.0, 0.0), flags=L.PBC_ALL, ranges=None, pooled=None, device=False, mass=None):
    import cases
    F, _, N = coords.shape
    cell = V.make_unitcell(box, flags, tilt)
    ev = V.ScriptEval(F, ir)
    sysm = V.MolSystem(N, mass=mass, unitcell=cell)
    traj = cases.make_traj(lib, coords, cell, device)
    for beg, end in (ranges or [(0, F)]):
        assert (ev.frame_range_pooled(sysm, traj, beg, end, *pooled) if pooled else ev.frame_range(sysm, traj, beg, end))
    assert ev.frame_mask().all()
    return ev


def counts_of(lib, props, coords, box, **kw):
    """props: [(name, T, R, rmin, rmax)] -> {name: float32 [F]}, after checking the shape of the record"""
    ir = V.ScriptIR(lib)
    for name, t, r, rmin, rmax in props:
        ir.add_within_count(name, t, r, rmin, rmax)
    ev = evaluate(lib, ir, coords, box, **kw)
    out = {}
    for name, *_ in props:
        pd = ev.property_data(name)
        assert tuple(pd.dim[:2]) == (coords.shape[0], 1) and pd.unit_str == ("", "")
        out[name] = rows(ev, name)[:, 0]
    return out


def both_kernels(lib, props, coords, box, **kw):
    """the evaluator with and without a grid: asserted from the profile counters; -> (pencil rows, brute rows)"""
    res = []
    for fb in (0, 1):
        lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
        try:
            with options(lib, force_brute=fb):
                res.append(counts_of(lib, props, coords, box, **kw))
        finally:
            lib.vmd_profile_enable(False)
        assert launches(lib, "within_brute" if fb else "within_pencil") >= len(props), fb
        assert launches(lib, "within_pencil" if fb else "within_brute") == 0, fb
    for name in res[0]:
        assert np.array_equal(res[0][name], res[1][name]), name
    return res[0]


def one(lib, pts, t, r, rmin, rmax, box=50.0, **kw):
    """one frame of a few points -> the count, from both paths where a grid exists"""
    xyz = np.asarray(pts, np.float32).T.copy()[None]
    a = counts_of(lib, [("n", t, r, rmin, rmax)], xyz, box, **kw)["n"]
    with options(lib, force_brute=1):
        b = counts_of(lib, [("n", t, r, rmin, rmax)], xyz, box, **kw)["n"]
    bx = Box(tuple(np.atleast_1d(box)) * (3 if np.isscalar(box) else 1) + tuple(kw.get("tilt", ())), kw.get("flags", 7))
    closed = bool(lib.vmd_set_option(b"spec_within_closed", 0))
    lib.vmd_set_option(b"spec_within_closed", int(closed))
    excl = bool(lib.vmd_set_option(b"spec_within_exclude_ref", 0))
    lib.vmd_set_option(b"spec_within_exclude_ref", int(excl))
    want = W.counts(xyz, (bx.L[0], bx.L[1], bx.L[2], bx.xy, bx.xz, bx.yz), t, r, rmin, rmax, closed=closed, exclude_ref=excl,
                    flags=kw.get("flags", 7))
    assert a[0] == b[0] == want[0], (a, b, want)
    return int(a[0])


# ---- 1. known answers ------------------------------------------------------------------------------------------------------------------

def known_answers(lib, device=False):
    kw = dict(device=device)
    pair = [(1.0, 5.0, 5.0), (4.0, 5.0, 5.0)]                                   # d == 3.0f exactly
    assert one(lib, pair, [0], [1], 0.0, 3.0, **kw) == 0                        # open above
    assert one(lib, pair, [0], [1], 3.0, 5.0, **kw) == 1                        # closed below
    assert one(lib, pair, [0], [1], 0.0, np.nextafter(np.float32(3.0), np.float32(4.0)), **kw) == 1
    with options(lib, spec_within_closed=1):
        assert one(lib, pair, [0], [1], 0.0, 3.0, **kw) == 1
        assert one(lib, pair, [0], [1], 3.0, 5.0, **kw) == 1
    seam = [(0.5, 7.0, 7.0), (49.0, 7.0, 7.0), (25.0, 25.0, 0.25), (25.0, 25.0, 49.0)]
    assert one(lib, seam, [0], [1], 0.0, 2.0, **kw) == 1                        # d = 1.5 across the periodic seam in x
    assert one(lib, seam, [2], [3], 0.0, 2.0, **kw) == 1                        # ... in z
    assert one(lib, seam, [2], [3], 0.0, 2.0, flags=3, **kw) == 0               # z open: 48.75 apart
    assert one(lib, seam, [0, 2], [1, 3], 0.0, 2.0, flags=3, **kw) == 1
    assert one(lib, seam, [0], [1], 0.0, 2.0, box=None, **kw) == 0              # no cell at all
    # a tilted cell: the nearest image lies one b vector (10, 20, 0) away
    skew = [(0.5, 0.5, 5.0), (10.25, 19.75, 5.0)]
    assert one(lib, skew, [0], [1], 0.0, 1.0, box=(20.0, 20.0, 20.0), tilt=(10.0, 0.0, 0.0), **kw) == 1
    assert one(lib, skew, [0], [1], 0.0, 1.0, box=(20.0, 20.0, 20.0), **kw) == 0
    # T == R: the scalar form saturates through d = 0 (D-WITHIN-SELF), the range form does not
    rng = np.random.default_rng(3)
    cloud = rng.uniform(0.0, 20.0, (300, 3))
    every = np.arange(300)
    assert one(lib, cloud, every, every, 0.0, 1.5, box=20.0, **kw) == 300
    n = one(lib, cloud, every, every, 0.5, 1.5, box=20.0, **kw)
    assert 0 < n < 300
    with options(lib, spec_within_exclude_ref=1):
        assert one(lib, cloud, every, every, 0.0, 1.5, box=20.0, **kw) == 0      # T minus R is empty: 0, never an error
        m = one(lib, cloud, every[:200], every[100:], 0.0, 1.5, box=20.0, **kw)  # the 100 atoms outside R
        assert 0 < m <= 100
    assert one(lib, cloud, every[:200], every[100:], 0.0, 1.5, box=20.0, **kw) >= 100 + m


def test_known_answers_on_the_emulator(emu_lib):
    known_answers(emu_lib)


# ---- 2. exactness at the interval ends ---------------------------------------------------------------------------------------------------

def steps(v, lo=-4, hi=4):
    out = []
    for k in range(lo, hi):
        x = np.float32(v)
        for _ in range(abs(k)):
            x = np.nextafter(x, np.float32(np.inf if k > 0 else 0.0))
        out.append(x)
    return out


RADII = [1.0, 2.0, 3.0, 3.5, 0.1, 0.3, 1.0 / 3.0, 5.0, 7.25, 10.0, 12.0, 2.0 ** 0.5, 3.0 ** 0.5, 0.7, 1.9999999, 2.0000002,
         float(np.nextafter(np.float32(3.5), np.float32(4))), float(np.nextafter(np.float32(3.5), np.float32(3))), 6.0221, 4.7,
         1.0e-3, 2.0 ** -60, 1000.0, 30000.0]


def threshold_exactness(lib, device=False, radii=RADII):
    """targets whose distance from the one reference atom (at the origin) steps through the floats around r, along x and along a
    3-4-5 diagonal: r as the upper end (scalar form) and as the lower end (range form), both interval rules, both paths"""
    checked = 0
    for r in radii:
        r = np.float32(r)
        pts = [(0.0, 0.0, 0.0)] + [(x, 0.0, 0.0) for x in steps(r)] + [(x, np.float32(0.8) * r, 0.0) for x in steps(np.float32(0.6) * r)]
        xyz = np.asarray(pts, np.float32).T.copy()[None]
        box = float(np.float32(12.0) * r)            # a few dozen pencils whatever r is: the grid path wherever choose_grid grants one
        props = [(f"s{t}", [t], [0], 0.0, float(r)) for t in range(1, len(pts))] + \
                [(f"r{t}", [t], [0], float(r), float(np.float32(2.0) * r)) for t in range(1, len(pts))]
        for closed in (0, 1):
            with options(lib, spec_within_closed=closed):
                got = counts_of(lib, props, xyz, box, device=device)
                with options(lib, force_brute=1):
                    brute = counts_of(lib, props, xyz, box, device=device)
            want = {n: W.counts(xyz, box, t, ref, a, b, closed=bool(closed)) for n, t, ref, a, b in props}
            for n in want:
                assert got[n][0] == brute[n][0] == want[n][0], (float(r), closed, n)
            s = np.array([want[f"s{t}"][0] for t in range(1, len(pts))])
            checked += 1
            if r > 1e-10:
                assert 0 < s[:8].sum() < 8, (float(r), s)              # the steps along x do straddle the end
    return checked


def test_threshold_exactness_on_the_emulator(emu_lib):
    assert threshold_exactness(emu_lib) == 2 * len(RADII)


# ---- 3. both kernels, same inputs --------------------------------------------------------------------------------------------------------

def blob12k(oracle, F=2):
    import cases
    n, nb = 12001, 2000
    coords = cases.host_frames(oracle, 4, n, 50.0, F, n_blob=nb)
    topo = synth.water_box_topology(n, n_blob=nb)
    return coords, topo


def sets_of(topo):
    el, rn = np.asarray(topo.elements), np.asarray(topo.resnames)
    water = rn == "HOH"
    return dict(blob=np.nonzero(~water)[0].astype(np.int32), wo=np.nonzero(water & (el == "O"))[0].astype(np.int32),
                h=np.nonzero(el == "H")[0].astype(np.int32), water=np.nonzero(water)[0].astype(np.int32),
                all=np.arange(el.size, dtype=np.int32))


def varied(want, nt):
    """the non-saturation rule: asserted on the restatement's numbers"""
    assert ((want > 0) & (want < nt)).all() and len(set(want.tolist())) > 1, (want, nt)


def direct_brute(lib, xyz, box9, pbc, t, r, rmin, rmax, closed, gpu=False):
    """vmd_hip_within_brute through ctypes on one frame -> the count"""
    N = xyz.shape[1]
    t, r = np.ascontiguousarray(t, np.int32), np.ascontiguousarray(r, np.int32)
    frame = np.ascontiguousarray(xyz, np.float32)
    b9 = np.ascontiguousarray(box9, np.float32)
    if gpu:
        import torch
        d = [torch.from_numpy(a).cuda() for a in (frame, b9, t, r)]
        out = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ptr = [x.data_ptr() for x in d] + [out.data_ptr()]
    else:
        out = np.full(1, 77, np.uint32)
        ptr = [a.ctypes.data for a in (frame, b9, t, r)] + [out.ctypes.data]
    rc = lib.vmd_hip_within_brute(None, ptr[0], 3 * N, N, ptr[1], pbc, 1, ptr[2], t.size, ptr[3], r.size, rmin, rmax, closed, ptr[4])
    assert rc == 0
    if gpu:
        torch.cuda.synchronize()
        return int(out.cpu().numpy()[0])
    return int(out[0])


def box9(box, tilt=(0.0, 0.0, 0.0)):
    b = np.float32(box) if not np.isscalar(box) else np.float32([box] * 3)
    return np.concatenate([b, np.float32(1.0) / b, np.float32(tilt)]).astype(np.float32)


def kernels_on_the_blob(lib, oracle, device=False, F=2):
    coords, topo = blob12k(oracle, F)
    s = sets_of(topo)
    props = [("a", s["wo"], s["blob"], 0.0, 3.5), ("b", s["wo"], s["wo"], 0.5, 2.0), ("c", s["all"], s["blob"], 0.0, 3.0)]
    cells = [dict(box=50.0), dict(box=(50.0, 50.0, 50.0), tilt=TILT), dict(box=50.0, flags=3)]
    for cell in cells:
        tri = "tilt" in cell
        b6 = tuple(np.atleast_1d(cell["box"])) * (1 if tri else 3) + cell.get("tilt", (0.0, 0.0, 0.0))
        flags = cell.get("flags", 7)
        want = {n: W.counts(coords, b6, t, r, a, b, flags=flags, slab=True, frames=[0] if tri and n != "a" else None)
                for n, t, r, a, b in props}
        for n, t, *_ in props:
            if len(want[n]) > 1:
                varied(want[n], len(t))
        for small in (0, 8192):            # 0: every selection through the pencil buckets; 8192: the blob by one block per frame in LDS
            with options(lib, cells_small=small):
                got = both_kernels(lib, props, coords, device=device, **cell)
            for n in want:
                assert np.array_equal(got[n][:len(want[n])], want[n]), (cell, small, n, got[n], want[n])
        if flags == 7:
            pbc = 7 | (8 if tri else 0)
            n, t, r, a, b = props[0]
            assert direct_brute(lib, coords[0], box9(cell["box"], cell.get("tilt", (0.0, 0.0, 0.0))), pbc, t, r, a, b, 0, gpu=device) == want[n][0]
    one_frame = W.counts(coords[:1], 50.0, s["wo"], s["blob"], 0.0, 3.5)
    assert one_frame[0] == W.counts(coords[:1], 50.0, s["wo"], s["blob"], 0.0, 3.5, slab=True)[0]      # the shortcut changes nothing
    f64 = W.count64(coords[0], Box(50.0), s["wo"], s["blob"], 0.0, 3.5)
    print(f"water O within 3.5 of the blob, frame 0: fp32 contract {int(one_frame[0])}, float64 minimum image {f64}")


def test_both_kernels_on_the_blob_system(emu_lib, oracle):
    kernels_on_the_blob(emu_lib, oracle)


def test_self_rule_on_the_blob_system(emu_lib, oracle):
    coords, topo = blob12k(oracle, 2)
    o = np.nonzero(np.asarray(topo.elements) == "O")[0].astype(np.int32)
    got = both_kernels(emu_lib, [("n", o, o, 0.0, 3.5)], coords, 50.0)["n"]
    assert (got == o.size).all()
    with options(emu_lib, spec_within_exclude_ref=1):
        assert not counts_of(emu_lib, [("n", o, o, 0.0, 3.5)], coords, 50.0)["n"].any()


def brute_tile_edges(lib, device=False):
    """the all-pairs loop at the edges of its 256-wide tile of R: one frame, a cubic periodic box of edge 60, range 0:2.0.  T: 130 atoms
    3.0 apart on a line that winds through the cell in the plane z = 10 (three waves of the 64-wide kernel, more than half a block of the
    256-wide one).  R: nref atoms parked in the plane z = 40, 30 from every target, but for ONE planted entry 1.0 above one target.
    vmd_hip_within_brute, _brute_flags, _brute_atoms and _brute_expr (term 2, every lane live, the bytes preset to 1), and
    vmd_hip_within_brute once more without a reference list (R are the frame's first atoms: NULL names them) -> cases checked"""
    box, rmin, rmax, nt = 60.0, 0.0, 2.0, 130
    bx = Box((box,) * 3 + (0.0,) * 3, 7)
    step_y = 0.18                                      # the line passes itself 20 steps on, 3.6 further up: no two targets closer than 3.0
    i = np.arange(nt)
    tgt = np.stack([(1.0 + i * np.sqrt(9.0 - step_y ** 2)) % box, 5.0 + i * step_y, np.full(nt, 10.0)]).astype(np.float32)
    d = tgt[:, :, None] - tgt[:, None, :]
    d -= box * np.rint(d / box)
    assert np.sqrt((d * d).sum(0))[~np.eye(nt, dtype=bool)].min() > 2.999
    cases, checked = [], 0
    for nref in (1, 255, 256, 257, 512, 513):
        cases += [(nref, j) for j in sorted({0, nref - 1} | {j for j in (255, 256) if j < nref})]
    cases.append((257, None))
    for nref, planted in cases:
        N = nt + nref
        R, T = np.arange(nref, dtype=np.int32), np.arange(nref, N, dtype=np.int32)
        k = np.arange(nref)
        xyz = np.concatenate([np.stack([1.0 + 0.25 * (k % 32), 1.0 + 0.25 * (k // 32), np.full(nref, 40.0)]).astype(np.float32), tgt], axis=1)
        at = None
        if planted is not None:
            at = (0, 63, 64, 129)[checked % 4]
            xyz[:, planted] = tgt[:, at] + np.float32([0.0, 0.0, 1.0])
        xyz = np.ascontiguousarray(xyz, np.float32)
        want = np.zeros(nt, bool)
        if at is not None:
            want[at] = True
        # the placement, from the restatement alone: exactly the planted member
        assert np.array_equal(W.hits(xyz, bx, T, R, rmin, rmax, False, False), want), (nref, planted, at)
        host = dict(xyz=xyz, b9=box9(box), T=T, R=R, cnt=np.full(4, 77, np.uint32), fl=np.full(nt, 9, np.uint8), mb=np.zeros(N, np.uint8),
                    bits=np.ones(N, np.uint8))
        if device:
            import torch
            dev = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in host.items()}
            torch.cuda.synchronize()
            p = {k: v.data_ptr() for k, v in dev.items()}
        else:
            p = {k: v.ctypes.data for k, v in host.items()}
        head = (None, p["xyz"], 3 * N, N, p["b9"], 7, 1, p["T"], nt, p["R"], nref, rmin, rmax, 0)
        assert lib.vmd_hip_within_brute(*head, p["cnt"]) == 0
        assert lib.vmd_hip_within_brute_flags(*head, p["cnt"] + 4, p["fl"]) == 0
        assert lib.vmd_hip_within_brute_atoms(*head, p["cnt"] + 8, p["mb"], N) == 0
        assert lib.vmd_hip_within_brute_expr(*head, 2, 0xffff, p["bits"], N, None) == 0
        assert lib.vmd_hip_within_brute(*head[:9], None, *head[10:], p["cnt"] + 12) == 0
        if device:
            torch.cuda.synchronize()
            out = {k: dev[k].cpu().numpy() for k in ("cnt", "fl", "mb", "bits")}
        else:
            out = host
        what = (nref, planted, at)
        by_atom = np.zeros(N, bool); by_atom[nref:] = want
        assert [int(v) for v in out["cnt"]] == [int(want.sum())] * 4, (what, out["cnt"])
        assert np.array_equal(out["fl"], want.astype(np.uint8)), what
        assert np.array_equal(out["mb"], by_atom.astype(np.uint8)), what
        assert np.array_equal(out["bits"], np.where(by_atom, 1 | 4, 1).astype(np.uint8)), what
        checked += 1
    return checked


def test_brute_tile_edges_on_the_emulator(emu_lib):
    assert brute_tile_edges(emu_lib) == 17


# ---- 4. script level ---------------------------------------------------------------------------------------------------------------------

BLOB_SCRIPT = ("a = count(water and element('O') and within(3.5, not water));\n"
               "b = count(water and element('O') and within(0.5:2.0, water and element('O')));\n"
               "c = count(water and element('O') and within(1.2:1.8, element('H')));\n"
               "d = count(all and within(3.0, not water));\n"
               "e = count(water and within(2.0:4.0, not water));")


def script_parity(lib, coords, topo, text, box, device=False, frames=None, slab=True):
    ir, info = script.compile_script(text, topo, lib=lib, within=True)
    ir_c = script.compile_script_native(text, topo, lib=lib, within=True)
    assert ir.fingerprint() == ir_c.fingerprint() and ir.property_names() == ir_c.property_names()
    ev = evaluate(lib, ir_c, coords, box, device=device)
    frames = list(range(coords.shape[0])) if frames is None else frames
    for name, i in info.items():
        assert i["kind"] == "within_count"
        want = W.counts(coords, box, i["target"], i["ref"], i["rmin"], i["rmax"], frames=frames, slab=slab)
        varied(want, len(i["target"]))
        got = rows(ev, name)[:, 0]
        print(name, len(i["target"]), want)
        assert np.array_equal(got[frames], want), (name, got[frames], want)
    return info


def test_scripts_on_the_emulator(emu_lib, oracle):
    coords, topo = blob12k(oracle, 3)
    info = script_parity(emu_lib, coords, topo, BLOB_SCRIPT, 50.0)
    assert [len(info[n]["target"]) for n in "abcde"] == [3334, 3334, 3334, 12001, 10001]
    import cases
    box_coords = cases.water_box(oracle, 2, 3000, 31.0, 4)
    script_parity(emu_lib, box_coords, synth.water_box_topology(3000), "n = count(element('O') and within(3.5, atom(1:30)));", 31.0)


# ---- 5. against rdf() --------------------------------------------------------------------------------------------------------------------

def rdf_cross_check(lib, oracle, device=False):
    """R = one atom outside T: a target is hit iff its one pair is in range, so the counts sum to the rdf histogram's total"""
    import cases
    coords = cases.water_box(oracle, 2, 3000, 31.0, 4)
    t = cases.oxygen(3000)[1:]
    ref = np.array([1], np.int32)
    r = 6.0
    d = np.concatenate([W.pair_d(Box(31.0), W.wrap(c[:, t], Box(31.0))[:, :, None], W.wrap(c[:, ref], Box(31.0))[:, None, :]).ravel() for c in coords])
    assert (d != 0).all() and (d != np.float32(r)).all()               # open and closed ends agree on these inputs
    ir = V.ScriptIR(lib)
    ir.add_within_count("n", t, ref, 0.0, r)
    ir.add_rdf("g", ref, t, (0.0, r))
    ev = evaluate(lib, ir, coords, 31.0, device=device)
    total = int(ev.property_data("g").counts.sum())
    assert total == int(rows(ev, "n").sum()) == int((d < np.float32(r)).sum()) and total > 0


def test_cross_check_against_rdf(emu_lib, oracle):
    rdf_cross_check(emu_lib, oracle)


# ---- 6. call patterns --------------------------------------------------------------------------------------------------------------------

CALL_SCRIPT = ("a = count(water and element('O') and within(3.5, not water)); g = rdf(element('O'), element('O'), 3.5);"
               "b = count(element('O') and within(0.5:2.0, element('O'))); d = distance(10, 30);")
CALL_NAMES = ("a", "b", "d")
RAGGED = [(0, 7), (7, 8), (8, 21), (21, 30)]


def call_patterns(lib, oracle, device=False):
    coords, topo = TG.blob_system(oracle, n_atoms=3000, n_blob=200, F=30)
    ir = script.compile_script(CALL_SCRIPT, topo, lib=lib, within=True)[0]
    run = lambda **kw: evaluate(lib, ir, coords, 30.0, device=device, **kw)
    one_call = run()
    got = {"grain 1": run(pooled=(16, 1)), "grain 4": run(pooled=(4, 4)), "ragged": run(ranges=RAGGED), "late first": run(ranges=RAGGED[::-1])}
    for bf in (3, 16):
        with options(lib, batch_frames=bf):
            got[f"batch_frames {bf}"] = run()
    with options(lib, readahead=0):
        got["no read-ahead"] = run(pooled=(8, 1))
    with options(lib, force_brute=1):
        got["brute"] = run()
    got["resident" if not device else "host"] = evaluate(lib, ir, coords, 30.0, device=not device) if lib.vmd_device_count() > 0 else one_call
    # block partials and a filtered evaluation served from them
    full = V.ScriptEval(30, ir); full.set_block_frames(5)
    import cases
    cell = V.make_unitcell(30.0)
    sysm, traj = V.MolSystem(coords.shape[2], unitcell=cell), cases.make_traj(lib, coords, cell, device)
    assert full.frame_range(sysm, traj, 0, 30)
    got["block partials"] = full
    filt = V.ScriptEval(30, ir); filt.set_source(full)
    assert filt.frame_range(sysm, traj, 5, 22)
    for name in CALL_NAMES:
        assert bits_equal(rows(filt, name)[5:22], rows(one_call, name)[5:22]), name
    assert filt.frame_stats()[1] > 0
    for what, ev in got.items():
        for name in CALL_NAMES:
            assert bits_equal(rows(ev, name), rows(one_call, name)), (what, name)
        assert np.array_equal(ev.property_data("g").counts, one_call.property_data("g").counts), what
    a = rows(one_call, "a")[:, 0]
    assert len(set(a.tolist())) > 1 and (a > 0).all()
    # a cutoff above half the cell: no grid, all pairs, S3's single image
    o = np.nonzero(np.asarray(topo.elements) == "O")[0].astype(np.int32)
    lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
    try:
        wide = counts_of(lib, [("w", o[:40], np.arange(200, dtype=np.int32), 14.0, 16.0)], coords[:2], 30.0, device=device)["w"]
    finally:
        lib.vmd_profile_enable(False)
    assert launches(lib, "within_brute") >= 1 and launches(lib, "within_pencil") == 0
    assert np.array_equal(wide, W.counts(coords[:2], 30.0, o[:40], np.arange(200), 14.0, 16.0))
    stats = one_call.property_data("a")
    assert stats.values.shape[0] == 30


def test_call_patterns(emu_lib, oracle):
    call_patterns(emu_lib, oracle)


def overflow_case(lib, oracle, device=False):
    """the middle frames pile every oxygen into one pencil: a bucket sized from the batch's ends overflows, the batch is repeated"""
    import cases
    n, box, F = 3000, 60.0, 12
    coords = cases.water_box(oracle, 5, n, box, F)
    o = cases.oxygen(n)
    rng = np.random.default_rng(3)
    for f in (5, 6, 7):
        coords[f][:, o] = rng.uniform(1.0, 11.0, (3, o.size)).astype(np.float32)
    h = cases.hydrogen(n)
    props = [("n", o, h[::2], 0.0, 3.0), ("m", o, o, 1.0, 12.0)]
    want = {nm: W.counts(coords, box, t, r, a, b, slab=True) for nm, t, r, a, b in props}
    with options(lib, cells_small=0, cells_cap_sample=2):
        for bf, defer in ((0, 1), (4, 1), (4, 0)):
            with options(lib, batch_frames=bf, defer_sync=defer):
                ir = V.ScriptIR(lib)
                for nm, t, r, a, b in props:
                    ir.add_within_count(nm, t, r, a, b)
                ev = evaluate(lib, ir, coords, box, device=device)
                assert ev.cell_build_stats()[0] >= 1, (bf, defer)
                for nm in want:
                    assert np.array_equal(rows(ev, nm)[:, 0], want[nm]), (bf, defer, nm)


def test_a_bucket_overflow_repeats_the_batch(emu_lib, oracle):
    overflow_case(emu_lib, oracle)


ORDER_SCRIPT = ["n1 = count(element('O') and within(3.5, residue(1:10)));", "d = distance(1, 50);",
                "{lin,plan,iso} = shape_weights(all) in residue(1:100);", "n2 = count(element('O') and within(5.0, residue(1:10)));",
                "rm = rmsd(all) in residue(1:8);", "a = angle(2,1,3) in residue(1:100);", "dm = distance_min(1:2, element('O')) in residue(2:5);"]
ORDER_NAMES = ["n1", "d", "lin", "plan", "iso", "n2", "rm", "a", "dm"]
ORDER_WIDTHS = [1, 1, 100, 100, 100, 1, 8, 100, 4]


def row_order_case(lib, oracle, device=False):
    """temporal properties of every kind in an order no other script has them in, the within counts (whose rows leave from launch_rdf)
    first and in the middle, rows of 1, 4, 8 and 100 floats: every property's rows, bit for bit, are the rows it has as the only
    statement of an evaluator of its own - whether the batch's host slot is filled and read in batches of 3, 3, 2 (completed behind
    the next batch or at once), in one batch, or by pooled calls whose rows wait in ahead_values"""
    import cases
    n, box, F = 300, 20.0, 8
    coords = cases.water_box(oracle, 11, n, box, F)
    topo = synth.water_box_topology(n)
    opt_ins = dict(within=True, angles=True, shape=True, rmsd=True)
    want = {}
    with options(lib, batch_frames=0):
        for stmt in ORDER_SCRIPT:
            ir, info = script.compile_script(stmt, topo, lib=lib, **opt_ins)
            alone = evaluate(lib, ir, coords, box, device=device)
            for name in ir.property_names():
                want[name] = rows(alone, name)
                if info[name]["kind"] == "within_count":
                    i = info[name]
                    assert np.array_equal(want[name][:, 0], W.counts(coords, box, i["target"], i["ref"], i["rmin"], i["rmax"], slab=True)), name
    assert list(want) == ORDER_NAMES and [want[nm].shape for nm in ORDER_NAMES] == [(F, w) for w in ORDER_WIDTHS]
    assert not np.array_equal(want["n1"], want["n2"]) and len({want[nm].tobytes() for nm in ("lin", "plan", "iso", "a")}) == 4
    ir = script.compile_script("\n".join(ORDER_SCRIPT), topo, lib=lib, **opt_ins)[0]
    assert ir.property_names() == ORDER_NAMES
    settings = {"batches of 3, deferred": (dict(batch_frames=3, defer_sync=1), {}), "batches of 3": (dict(batch_frames=3, defer_sync=0), {}),
                "one batch": (dict(batch_frames=0), {}), "pooled, read ahead": (dict(readahead=1), dict(pooled=(8, 1)))}
    for what, (opts, kw) in settings.items():
        lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
        try:
            with options(lib, **opts):
                ev = evaluate(lib, ir, coords, box, device=device, **kw)
        finally:
            lib.vmd_profile_enable(False)
        if "batch_frames" in opts:
            assert launches(lib, "batches") == (3 if opts["batch_frames"] else 1), what
        for name in ORDER_NAMES:
            assert bits_equal(rows(ev, name), want[name]), (what, name)
    # whether a pool's calls meet in a read-ahead region is up to its threads; one caller walking frame by frame with the deferred settle
    # always does: blocks of 3, 3 and 2 frames evaluated ahead in one batch, their rows in ahead_values until the blocks are committed
    cell = V.make_unitcell(box)
    sysm, traj = V.MolSystem(n, unitcell=cell), cases.make_traj(lib, coords, cell, device)
    ev = V.ScriptEval(F, ir); ev.set_block_frames(3); ev.set_deferred_settle(1)
    for f in range(F):
        assert ev.frame_range(sysm, traj, f, f + 1)
    ev.wait_settled()
    st = ev.readahead_stats()
    assert ev.frame_mask().all() and st["regions"] >= 1 and st["region_frames"] == F and st["committed_blocks"] == 3, st
    for name in ORDER_NAMES:
        assert bits_equal(rows(ev, name), want[name]), ("evaluated ahead", name)


def test_rows_of_temporal_properties_in_an_unusual_order(emu_lib, oracle):
    row_order_case(emu_lib, oracle)


# ---- 7. multi-rank, export -----------------------------------------------------------------------------------------------------------------

MERGE_SCRIPT = "a = count(water and element('O') and within(3.5, not water)); d = distance(10, 30);"


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
    ir = script.compile_script(MERGE_SCRIPT, topo, lib=lib, within=True)[0]
    F = coords.shape[0]
    ev = V.ScriptEval(F, ir)
    beg, end = shard_frames(F, rank, world)
    cell = V.make_unitcell(30.0)
    assert ev.frame_range(V.MolSystem(coords.shape[2], unitcell=cell), V.HostTrajectory(coords, cell), beg, end)
    reduce_eval(ev)
    assert ev.frame_mask().all()
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), a=ev.property_data("a").values, d=ev.property_data("d").values)
    dist.destroy_process_group()


def test_multi_rank_merge(emu_lib, oracle, tmp_path):
    import torch.multiprocessing as mp
    port = 39500 + (os.getpid() % 2000)
    mp.spawn(_merge_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    coords, topo = TG.blob_system(oracle, n_atoms=3000, F=7)
    ir = script.compile_script(MERGE_SCRIPT, topo, lib=emu_lib, within=True)[0]
    one_rank = evaluate(emu_lib, ir, coords, 30.0)
    for r in range(2):
        z = np.load(tmp_path / f"rank{r}.npz")
        for n in ("a", "d"):
            assert bits_equal(z[n].reshape(7, -1), rows(one_rank, n)), n


def test_export_table(emu_lib, oracle, tmp_path):
    coords, topo = TG.blob_system(oracle, n_atoms=3000, F=5)
    ir = script.compile_script("nw = count(water and element('O') and within(3.5, not water));", topo, lib=emu_lib, within=True)[0]
    ev = evaluate(emu_lib, ir, coords, 30.0)
    y = rows(ev, "nw")[:, 0]
    for ext in ("xvg", "csv"):
        path = tmp_path / f"nw.{ext}"
        ev.export_table(path, "nw", ext)
        text = open(path, encoding="utf-8").read()
        assert "nw" in text, text[:400]
        nums = [ln.replace(",", " ").split() for ln in text.splitlines() if ln.strip() and ln.strip()[0] in "0123456789"]
        assert len(nums) == 5 and [float(ln[1]) for ln in nums] == y.tolist()


# ---- 8. front-end ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def topo():
    return synth.water_box_topology(200 + 933 * 3, n_blob=200)


OPT_INS = dict(angles=True, shape=True, rmsd=True)


def test_without_the_opt_in_nothing_changes(host_lib, topo):
    import test_rmsd
    assert test_rmsd._old_ir(host_lib).fingerprint() == test_rmsd.PARENT_FINGERPRINT          # the literal the parent's suite holds
    text = VIAMD_DEFAULT_SCRIPT + NW_LINE
    ir_a, rep_a = script.compile_script_native(text, topo, lib=host_lib, partial=True, **OPT_INS)
    ir_b, rep_b = script.compile_script_native(text, topo, lib=host_lib, partial=True, within=False, **OPT_INS)
    ir_py, _, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, within=False, **OPT_INS)
    assert ir_a.property_names() == ir_b.property_names() == ir_py.property_names() == ["d1", "a1", "r", "v", "lin", "plan", "iso"]
    assert ir_a.fingerprint() == ir_b.fingerprint() == ir_py.fingerprint() and rep_a == rep_b == rep_py
    k = rep_a["skipped"][0]
    assert [s["names"] for s in rep_a["skipped"]] == ["nw"] and text[k["beg"]:k["end"]] == NW_LINE[1:-1]
    assert k["reason"] == "unsupported function 'count' (outside the rdf / sdf / distance path)"      # the parent commit's words
    # scripts without the statement keep their fingerprints and reports whatever the new bit says
    for text0, kw in ((VIAMD_DEFAULT_SCRIPT, OPT_INS), (VIAMD_DEFAULT_SCRIPT, {}), (VIAMD_DEFAULT_SCRIPT + '\nrm = rmsd(resname("ALA"));', OPT_INS),
                      ("x = within(3, all); y = rdf(within(3, all), all, 5.0); d = distance(1, 2);", {})):
        res = [script.compile_script_native(text0, topo, lib=host_lib, partial=True, within=w, **kw) for w in (False, True)]
        res.append(script.compile_script(text0, topo, lib=host_lib, partial=True, within=True, **kw)[::2])
        assert len({r[0].fingerprint() for r in res}) == 1 and res[0][1] == res[1][1] == res[2][1], text0
    for compiler in (script.compile_script_native, script.compile_script):
        for stmt, fn in (("n = count(all and within(3, water));", "count"), ("s = within(3, water);", "within")):
            with pytest.raises(script.ScriptError) as err:
                compiler(stmt, topo, lib=host_lib, **OPT_INS)
            assert str(err.value) == f"unsupported function '{fn}' (outside the rdf / sdf / distance path)"


def test_default_script_with_the_four_opt_ins(host_lib, topo):
    text = VIAMD_DEFAULT_SCRIPT + NW_LINE
    ir_c, rep_c = script.compile_script_native(text, topo, lib=host_lib, partial=True, within=True, **OPT_INS)
    ir_py, info, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, within=True, **OPT_INS)
    assert ir_c.property_names() == ir_py.property_names() == ["d1", "a1", "r", "v", "lin", "plan", "iso", "nw"]
    assert ir_c.fingerprint() == ir_py.fingerprint() and ir_c.property_flags("nw") == L.FLAG_TEMPORAL
    assert rep_c == rep_py and rep_c["skipped"] == []
    fb = rep_c["fallback_source"]
    assert len(fb) == len(text) and fb.strip() == 's1 = resname("ALA")[2:8];'
    i = info["nw"]
    assert i["kind"] == "within_count" and (i["rmin"], i["rmax"]) == (0.0, 3.5)
    assert list(i["ref"]) == list(range(200)) and len(i["target"]) == 20 + 933
    assert list(ir_c.geometry_atoms("nw")) == list(i["ref"]) + list(i["target"])
    strict = script.compile_script_native(text, topo, lib=host_lib, within=True, **OPT_INS)
    assert strict.fingerprint() == ir_c.fingerprint()


ACCEPTED = [
    ("n = count(within(3.5, resname(\"ALA\")));", 2999, 200, 0.0, 3.5),                      # no static factor: all atoms
    ("n = count(within(3.5:5.0, protein) and water);", 2799, 200, 3.5, 5.0),
    ("n = count(water and within(2, atom(1:30)) and element('O'));", 933, 30, 0.0, 2.0),
    ("n = count((element('O') or element('N')) and not water and within(1.5, (water)));", 40, 2799, 0.0, 1.5),
    ("s = resname(\"ALA\")[2:8]; n = count(element('H') and within(0.5:2.5, s));", 80 + 1866, 70, 0.5, 2.5),
]

SKIPPED = [
    ("n = count(water and not within(3, protein));", "within() must be a factor of the top-level AND"),
    ("n = count(water or within(3, protein));", "within() must be a factor of the top-level AND"),
    ("n = count(water and (within(3, protein)));", "within() must be a factor of the top-level AND"),
    ("n = count(within(3, protein) and within(5, water));", "count takes exactly one within() factor, found 2"),
    ("n = count(water and within(3, within(4, protein)));", "count takes exactly one within() factor, found 2"),
    ("n = count(water and within(3, protein)) in resname(\"ALA\");", "count(...) in <contexts> is outside the subset"),
    ("n = count(water);", "count of a static selection is a constant (left to the fallback)"),
    ("n = rdf(within(3, protein), water, 5.0);", "unsupported function 'within'"),
    ("n = sdf(resname(\"ALA\"), within(3, protein), 5.0);", "unsupported function 'within'"),
    ("n = distance(within(3, protein), water);", "unsupported function 'within'"),
    ("n = count(resname(\"XYZ\") and within(3, protein));", "n: empty selection"),
    ("n = count(water and within(3, resname(\"XYZ\")));", "n: empty selection"),
    ("n = count(water and within(0, protein));", "within needs a radius > 0"),
    ("n = count(water and within(0.0, protein));", "within needs a radius > 0"),
    ("n = count(water and within(5:3, protein));", "within range needs 0 <= a < b"),
    ("n = count(water and within(3:3, protein));", "within range needs 0 <= a < b"),
    ("n = count(water and within(3));", "expected ,"),
    ("n = count(water and within(protein, 3));", "expected num"),
    ("d = count(water and within(3, protein));", "already defined"),
]


@pytest.mark.parametrize("stmt,nt,nr,rmin,rmax", ACCEPTED)
def test_accepted_forms(host_lib, topo, stmt, nt, nr, rmin, rmax):
    ir_c = script.compile_script_native(stmt, topo, lib=host_lib, within=True)
    ir_py, info = script.compile_script(stmt, topo, lib=host_lib, within=True)
    assert ir_c.property_names() == ir_py.property_names() == ["n"] and ir_c.fingerprint() == ir_py.fingerprint()
    i = info["n"]
    assert (len(i["target"]), len(i["ref"]), i["rmin"], i["rmax"]) == (nt, nr, rmin, rmax)
    assert list(ir_c.geometry_atoms("n")) == list(i["ref"]) + list(i["target"])
    assert int(host_lib.vmd_ir_work_per_frame(ir_c.h)) == nt + nr


@pytest.mark.parametrize("stmt,reason", SKIPPED)
def test_skipped_forms(host_lib, topo, stmt, reason):
    text = "d = distance(1, 2);\n" + stmt + "\ne = distance(3, 4);"
    for compiler in (script.compile_script_native, script.compile_script):
        with pytest.raises((script.ScriptError, V.VmdError)) as err:
            compiler(text, topo, lib=host_lib, within=True)
        assert reason in str(err.value)
    ir_c, rep_c = script.compile_script_native(text, topo, lib=host_lib, partial=True, within=True)
    ir_py, _, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, within=True)
    assert ir_c.property_names() == ir_py.property_names() == ["d", "e"] and ir_c.fingerprint() == ir_py.fingerprint()
    assert rep_c == rep_py and len(rep_c["skipped"]) == 1
    k = rep_c["skipped"][0]
    assert k["names"] == stmt.split(" ")[0] and reason in k["reason"] and text[k["beg"]:k["end"]] == stmt[:-1]
    assert stmt in rep_c["fallback_source"] and "distance(3, 4)" not in rep_c["fallback_source"]


# ---- 9. ABI --------------------------------------------------------------------------------------------------------------------------------

def test_ir_validation_errors(host_lib):
    lib = host_lib
    for sym in ("vmd_ir_add_within_count", "vmd_hip_within_brute", "vmd_hip_within_pencil", "vmd_hip_within_to_float"):
        assert hasattr(lib, sym), sym
    ir = V.ScriptIR(lib)
    for t, r, a, b, msg in (([], [1], 0.0, 3.0, "target set is empty"), ([0], [], 0.0, 3.0, "reference set is empty"), ([0, -1], [1], 0.0, 3.0, "negative"),
                            ([0], [1], 3.0, 3.0, "0 <= rmin < rmax"), ([0], [1], -1.0, 3.0, "0 <= rmin < rmax"), ([0], [1], 0.0, float("inf"), "finite"),
                            ([0], [1], float("nan"), 3.0, "finite"), ([0], [1], 0.0, 0.0, "0 <= rmin < rmax")):
        with pytest.raises(V.VmdError, match=msg):
            ir.add_within_count("n", t, r, a, b)
    with pytest.raises(V.VmdError, match="name is empty"):
        ir.add_within_count("", [0], [1], 0.0, 3.0)
    assert ir.property_count() == 0
    ir.add_distance("d", [0], [1])
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_within_count("d", [0], [1], 0.0, 3.0)
    ir.add_within_count("n", [0, 5, 7], [1, 5], 0.5, 3.0)
    assert ir.property_names() == ["d", "n"] and ir.property_flags("n") == L.FLAG_TEMPORAL
    assert list(ir.geometry_atoms("n")) == [1, 5, 0, 5, 7] and list(ir.geometry_atoms("n", 0)) == [1, 5, 0, 5, 7]
    assert ir.geometry_atoms("n", 1).size == 0 and ir.geometry_atoms("d").size == 0
    assert int(lib.vmd_ir_work_per_frame(ir.h)) == 1 + 5
    a = np.array([0, 1], np.int32)
    p = lambda x: x.ctypes.data_as(L.c_int32_p)
    for kind in (4, 7, 8):
        assert not lib.vmd_ir_add_distance(ir.h, b"k", kind, p(a), 2, p(a), 2) and "unknown distance kind" in lib.last_error()

    def fp(*args):
        q = V.ScriptIR(lib)
        q.add_within_count(*args)
        return q.fingerprint()
    base = ("n", [0, 1, 2], [3, 4], 0.0, 3.0)
    variants = [base, ("m",) + base[1:], ("n", [0, 1], [3, 4], 0.0, 3.0), ("n", [0, 1, 2], [3], 0.0, 3.0), ("n", [0, 1, 2], [3, 4], 0.5, 3.0),
                ("n", [0, 1, 2], [3, 4], 0.0, 3.5), ("n", [3, 4], [0, 1, 2], 0.0, 3.0)]
    q = V.ScriptIR(lib); q.add_rdf("n", [3, 4], [0, 1, 2], (0.0, 3.0))
    assert len({fp(*v) for v in variants} | {q.fingerprint()}) == len(variants) + 1
    ir2 = V.ScriptIR(lib)
    ir2.add_within_count("n", [0, 99], [1], 0.0, 3.0)
    if lib.vmd_device_count() > 0:
        with pytest.raises(V.VmdError, match="references atom 99"):
            TG.evaluate(lib, ir2, np.zeros((1, 3, 10), np.float32), 10.0)


# ---- 10. VIAMD's default script plus the hydration-number line through the shim ---------------------------------------------------------------

def build_shim_within():
    """tests/native/shim_default_script_within.cpp linked against the product library"""
    return native_host.build_shim("shim_default_script_within")


def test_shim_default_script_with_the_within_line_on_the_emulator(emu_lib, tmp_path):
    import conftest
    exe = native_host.build_shim("shim_default_script_within", conftest.build_emu(), tmp_path / "shim_within_emu")
    native_host.run_ok([exe, "8"], "OK frames=8 properties=8 nw=gpu fallback_frame_range_calls=0")
    out = native_host.run_ok([exe, "8", "nobit"], "OK frames=8 properties=8 nw=fallback")
    assert "fallback_frame_range_calls=0" not in out.stdout, out.stdout
