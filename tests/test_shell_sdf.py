"""sdf() over a within() shell and shell masks in atom order on the emulator build and in the host-only entry points: known
answers, the mask of k_within_atoms against k_within_brute<true> and the numpy restatement at the shell radius, walk == all pairs == the
yardstick (tests/shell_sdf_ref.py) on the 12 001-atom blob system in three kinds of cell, identities that need no yardstick, call
patterns, a pencil-bucket overflow, co-evaluation with static properties, a two-rank merge, the opt-in front-end (C++ and Python twin),
ABI validation, vmd_eval_shell_mask and VIAMD's default script plus a shell sdf line through the shim.  Voxel counts, masks and
populations are integers: every comparison is `==`."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import native_host

import viamd_amd as V
from viamd_amd import _lib as L
from viamd_amd import script, synth

import shell_sdf_ref as S
import within_ref as W
import test_geometry as TG
import test_within as TW
import test_shell_rdf as TR
from geometry_ref import Box
from test_within import options, launches, evaluate, TILT, blob12k, sets_of, varied

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIAMD_DEFAULT_SCRIPT = TG.VIAMD_DEFAULT_SCRIPT
GS_LINE = "\ngs = sdf(s1, element('O') and within(3.5, resname(\"ALA\")), 10.0);"
WALK_KEYS = ("shell_mask", "cells_build")
BRUTE_KEYS = ("shell_mask_brute",)
ALL_BITS = dict(angles=True, shape=True, rmsd=True, within=True, shell_rdf=True, shell_sdf=True)


def make_ir(lib, props):
    """props: [(name, structures [K, m], T, shell | None, cutoff)], shell = (R, r_min, r_max)"""
    ir = V.ScriptIR(lib)
    for name, st, t, shell, cutoff in props:
        ir.add_sdf_shell(name, st, t, cutoff, target_shell=shell)
    return ir


def run(lib, props, coords, box, **kw):
    return evaluate(lib, make_ir(lib, props), coords, box, **kw)


def profiled(lib, fn, **opt):
    lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
    try:
        with options(lib, **opt):
            out = fn()
    finally:
        lib.vmd_profile_enable(False)
    return out, {k: launches(lib, k) for k in WALK_KEYS + BRUTE_KEYS + ("sdf_scatter",)}


def both_paths(lib, props, coords, box, **kw):
    """the evaluator on the walk and on all pairs, each FORCED (which one a shell gets by itself is a rule on |R|: mask_rule) and asserted
    from the profile counters -> (walk eval, all-pairs eval)"""
    ev_w, n_w = profiled(lib, lambda: run(lib, props, coords, box, **kw), shell_brute_below=0)
    assert all(n_w[k] >= 1 for k in WALK_KEYS) and n_w["shell_mask_brute"] == 0 and n_w["sdf_scatter"] >= 1, n_w
    ev_b, n_b = profiled(lib, lambda: run(lib, props, coords, box, **kw), force_brute=1)
    assert n_b["shell_mask_brute"] >= 1 and n_b["shell_mask"] == 0 and n_b["sdf_scatter"] >= 1, n_b
    for name, *_ in props:
        assert np.array_equal(vol(ev_w, name), vol(ev_b, name)), name
    return ev_w, ev_b


def vol(ev, name):
    return np.asarray(ev.property_data(name).counts)


def check(ev, name, want, cutoff):
    """the record of an sdf, against the yardstick's volume"""
    pd = ev.property_data(name)
    assert tuple(pd.dim) == (1, 128, 128, 128) and pd.min_range[0] == -np.float32(cutoff) and pd.max_range[0] == np.float32(cutoff)
    np.testing.assert_array_equal(pd.counts, want, err_msg=f"{name}: voxel counts differ from the yardstick")
    np.testing.assert_array_equal(pd.values, want.astype(np.float32))
    assert pd.max_value == float(want.max())


def caps(want, pops, static, nt):
    """what keeps a comparison from passing on nothing - asserted on the YARDSTICK's numbers before anything is compared"""
    varied(np.asarray(pops), nt)
    assert want.sum() > 0
    assert (want <= static).all() and not np.array_equal(want, static)


def blob_case(O, F=4):
    """the 12 001-atom blob system: the first four ALA residues are the structures, the water oxygens the target"""
    coords, topo = blob12k(O, F)
    s = sets_of(topo)
    return coords, topo, s, np.arange(40, dtype=np.int32).reshape(4, 10), np.asarray(topo.mass, np.float32)


# ---- 1. known answers ------------------------------------------------------------------------------------------------------------------

def known_answers(lib, O, device=False):
    """two rigid structures (atoms 0 - 3, 6 - 9: the same body 4 A apart), R = atom 4, targets: atom 0 (a member of structure 0, 2.5 from R),
    atom 5 (3.0 from R exactly), atom 10 (never near R); all three inside both cubes.  Frame 1 moves R away: an empty shell."""
    body = np.array([(1.0, 0.0, 0.0), (0.0, 1.5, 0.0), (0.0, 0.0, 0.7), (-1.0, -1.5, -0.7)])
    pts = np.zeros((11, 3))
    pts[0:4] = body + (20.0, 20.0, 20.0)
    pts[6:10] = body + (24.0, 20.0, 20.0)
    pts[4] = (21.0, 20.0, 22.5)
    pts[5] = (21.0, 23.0, 22.5)
    pts[10] = (25.0, 25.0, 25.0)
    f1 = pts.copy(); f1[4] = (40.0, 40.0, 40.0)
    xyz = np.ascontiguousarray(np.stack([pts, f1]).astype(np.float32).transpose(0, 2, 1))
    st = np.array([[0, 1, 2, 3], [6, 7, 8, 9]], np.int32)
    T, R = [0, 5, 10], [4]
    mass = np.ones(11, np.float32)
    up = float(np.nextafter(np.float32(3.0), np.float32(4.0)))

    def voxels(rlo, rhi, closed=0, include_self=0, frames=None):
        c = xyz if frames is None else xyz[frames]
        old = O.set_spec("sdf_include_self", include_self)
        try:
            with options(lib, spec_within_closed=closed, spec_sdf_include_self=include_self):
                evs = both_paths(lib, [("v", st, T, (R, rlo, rhi), 10.0)], c, 50.0, device=device, mass=mass)
            want, pops = S.shell_sdf(O, c, 50.0, st, mass, (T, (R, rlo, rhi)), 10.0, closed=bool(closed))
        finally:
            O.set_spec("sdf_include_self", old)
        check(evs[0], "v", want, 10.0)
        return int(vol(evs[0], "v").sum()), pops.tolist()
    # atom 0 is in: counted for structure 1, skipped for the structure it belongs to (D-SDF-EXCL); atom 5 at 3.0 is out of [0, 3.0)
    assert voxels(0.0, 3.0) == (1, [1, 0])
    assert voxels(0.0, up) == (3, [2, 0])                       # atom 5 is in: once per structure
    assert voxels(0.0, 3.0, closed=1) == (3, [2, 0])
    assert voxels(3.0, 5.0) == (2, [1, 0])                      # closed below: atom 5 alone
    assert voxels(0.0, up, include_self=1) == (4, [2, 0])       # spec_sdf_include_self: atom 0 for its own structure too
    # a frame with an empty shell adds no voxels and is an evaluated frame
    ev = run(lib, [("v", st, T, (R, 0.0, up), 10.0)], xyz[1:], 50.0, device=device, mass=mass)
    assert not vol(ev, "v").any() and ev.frame_mask().all() and ev.property_data("v").max_value == 0.0
    # the static sdf of the same list: every target for every structure but its own
    ev = run(lib, [("v", st, T, None, 10.0)], xyz, 50.0, device=device, mass=mass)
    assert int(vol(ev, "v").sum()) == 2 * 5


def test_known_answers_on_the_emulator(emu_lib, oracle):
    known_answers(emu_lib, oracle)


# ---- 2. the mask of k_within_atoms, at the kernels -------------------------------------------------------------------------------------------

def _grid(g9, pbc, rmax, split):
    """a pencil grid for one frame the way the evaluator cuts one: edges >= rmax / split (with its head room), fine cells <= rmax"""
    tri = bool(pbc & 8)
    Lx, Ly, Lz = (float(v) for v in g9[:3])
    xy, xz, yz = (float(v) for v in g9[6:9]) if tri else (0.0, 0.0, 0.0)
    w = [Lx, Ly / np.sqrt(1.0 + (yz / Lz) ** 2), Lz]
    n = [0, 0, 0]
    for a in (1, 2):
        redge = np.float32(rmax) / np.float32(split)
        k = int(np.floor(np.float32(w[a]) / redge))
        margin = np.float32(0.9999 if pbc & (1 << a) else 0.999)
        while k > 1 and (np.float32(k) / np.float32(w[a])) * redge > margin:
            k -= 1
        n[a] = min(max(k, 1), 1024)
    nxf = max(1, min(int(np.floor(np.float32(Lx) / np.float32(rmax))), 4096))
    return L.Grid(nxf, n[1], n[2], nxf * n[1] * n[2])


def kernel_masks(lib, xyz, box, T, R, rmin, rmax, closed=0, tilt=(0.0, 0.0, 0.0), flags=7, split=1, gpu=False):
    """one frame through vmd_hip_cells_build (R) + vmd_hip_within_atoms, vmd_hip_within_brute_atoms and vmd_hip_within_brute_flags ->
    (walk mask by atom, all-pairs mask by atom, all-pairs flags in list order, the three populations)"""
    N = xyz.shape[1]
    tri = any(tilt)
    pbc = flags | (8 if tri else 0)
    b9 = TW.box9(box, tilt)
    g9 = b9.copy()
    for a in range(3):
        if not (flags >> a) & 1:          # an open axis: the extent and origin of the bounding box, as the evaluator prepares them
            lo, hi = np.float32(xyz[a].min()), np.float32(xyz[a].max())
            pad = np.float32(max(1.0e-2, 1.0e-3 * float(hi - lo)))
            g9[6 + a] = lo - pad; g9[a] = (hi - lo) + np.float32(2.0) * pad; g9[3 + a] = np.float32(1.0) / g9[a]
    grid = _grid(g9, pbc, rmax, split)
    T, R = np.ascontiguousarray(T, np.int32), np.ascontiguousarray(R, np.int32)
    npad = (R.size + 63) & ~63
    words = int(lib.vmd_hip_cells_scratch_words(grid, int(R.size)))
    host = dict(xyz=np.ascontiguousarray(xyz, np.float32), b9=b9, g9=g9.astype(np.float32), T=T, R=R,
                cc=np.zeros(grid.ncell + 1, np.uint32), rank=np.zeros(max(words, 1), np.uint32), cs=np.zeros(grid.ncell + 1, np.uint32),
                srt=np.zeros(3 * npad + 64, np.float32), cnt=np.full(3, 77, np.uint32), mw=np.zeros(N, np.uint8), mb=np.zeros(N, np.uint8),
                fl=np.full(T.size, 9, np.uint8))
    if gpu:
        import torch
        dev = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in host.items()}
        torch.cuda.synchronize()
        p = {k: v.data_ptr() for k, v in dev.items()}
        esz = 4
    else:
        p = {k: v.ctypes.data for k, v in host.items()}
        esz = 4
    lib.vmd_hip_set_pencil_reach(split, split)
    try:
        assert lib.vmd_hip_cells_build(None, p["xyz"], 3 * N, N, p["g9"], pbc, 1, p["R"], R.size, npad, grid, p["cc"], p["rank"], p["cs"], p["srt"], None) == 0
        assert lib.vmd_hip_within_atoms(None, p["xyz"], 3 * N, N, p["g9"], pbc, 1, p["T"], T.size, p["srt"], p["cs"], R.size, npad, grid,
                                        rmin, rmax, closed, p["cnt"], p["mw"], N, None) == 0
    finally:
        lib.vmd_hip_set_pencil_reach(1, 1)
    assert lib.vmd_hip_within_brute_atoms(None, p["xyz"], 3 * N, N, p["b9"], pbc, 1, p["T"], T.size, p["R"], R.size, rmin, rmax, closed,
                                          p["cnt"] + esz, p["mb"], N) == 0
    assert lib.vmd_hip_within_brute_flags(None, p["xyz"], 3 * N, N, p["b9"], pbc, 1, p["T"], T.size, p["R"], R.size, rmin, rmax, closed,
                                          p["cnt"] + 2 * esz, p["fl"]) == 0
    if gpu:
        torch.cuda.synchronize()
        out = {k: dev[k].cpu().numpy() for k in ("mw", "mb", "fl", "cnt")}
    else:
        out = host
    return out["mw"].astype(bool), out["mb"].astype(bool), out["fl"].astype(bool), [int(v) for v in out["cnt"]]


def same_masks(lib, xyz, box, T, R, rmin, rmax, closed=0, tilt=(0.0, 0.0, 0.0), flags=7, split=1, gpu=False, what=""):
    """walk == all pairs (by atom and in list order) == the numpy restatement; -> the list-order hits"""
    mw, mb, fl, cnt = kernel_masks(lib, xyz, box, T, R, rmin, rmax, closed, tilt, flags, split, gpu)
    b = (box,) * 3 if np.isscalar(box) else tuple(box)
    want = W.hits(xyz, Box(tuple(float(v) for v in b) + tuple(float(v) for v in tilt), flags), T, R, rmin, rmax, bool(closed), not any(tilt))
    T = np.asarray(T)
    by_atom = np.zeros(xyz.shape[1], bool); by_atom[T[want]] = True
    assert np.array_equal(fl, want), what
    assert np.array_equal(mb, by_atom) and np.array_equal(mw, by_atom), (what, int(mw.sum()), int(mb.sum()), int(want.sum()))
    assert cnt == [int(want.sum())] * 3, (what, cnt)
    return want


def mask_exactness(lib, O, device=False, radii=TW.RADII):
    checked = 0
    # (a) the 24 radii of test_within, the targets stepping through the floats around r along x and along a 3-4-5 diagonal
    for r in radii:
        r = np.float32(r)
        pts = [(0.0, 0.0, 0.0)] + [(x, 0.0, 0.0) for x in TW.steps(r)] + [(x, np.float32(0.8) * r, 0.0) for x in TW.steps(np.float32(0.6) * r)]
        xyz = np.asarray(pts, np.float32).T.copy()
        box = float(np.float32(12.0) * r)
        T = np.arange(1, len(pts), dtype=np.int32)
        for closed in (0, 1):
            for split in (1, 2):
                s = same_masks(lib, xyz, box, T, [0], 0.0, float(r), closed, split=split, gpu=device, what=(float(r), closed, split, "upper"))
                same_masks(lib, xyz, box, T, [0], float(r), float(np.float32(2.0) * r), closed, split=split, gpu=device, what=(float(r), closed, split, "lower"))
                if r > 1e-10:
                    assert 0 < s[:8].sum() < 8, (float(r), s)          # the steps along x do straddle the end
        checked += 1
    # (b) a cloud in an orthorhombic, a tilted and a slab cell, single and split pencils; atoms far outside the cell are wrapped first
    rng = np.random.default_rng(17)
    n = 1500
    cloud = rng.uniform(-20.0, 60.0, (3, n)).astype(np.float32)
    T, R = np.arange(0, n, dtype=np.int32)[rng.permutation(n)[:900]], np.arange(0, n, 7, dtype=np.int32)
    # (flags 3: open z; flags 6: open x - the pencil axis itself is open there: its origin and padding, no image along x)
    for cell in (dict(box=40.0), dict(box=(40.0, 40.0, 40.0), tilt=TILT), dict(box=40.0, flags=3), dict(box=40.0, flags=6)):
        for split in (1, 2):
            for rmin, rmax in ((0.0, 3.5), (2.0, 4.0), (0.5, 1.9999999)):
                s = same_masks(lib, cloud, cell["box"], T, R, rmin, rmax, 0, cell.get("tilt", (0.0, 0.0, 0.0)), cell.get("flags", 7), split, device, what=(cell, split, rmax))
                assert 0 < s.sum() < T.size
                checked += 1
    # (c) atoms exactly on cell and pencil boundaries (k * edge for every k, in fp32, on every axis and on all three at once), plus their
    # neighbouring floats; the reference atoms a fixed offset away so that membership is decided across the boundary
    for split in (1, 2):
        box, rmax = 36.0, 3.0
        edges = np.arange(0, 13, dtype=np.float32) * np.float32(box / 12.0 / split)
        on = [(e, 7.3, 11.9) for e in edges] + [(7.3, e, 11.9) for e in edges] + [(7.3, 11.9, e) for e in edges] + [(e, e, e) for e in edges]
        on += [(np.nextafter(e, np.float32(-1)), np.nextafter(e, np.float32(99)), e) for e in edges[1:]]
        on += [(np.float32(box), np.float32(box), np.float32(box)), (np.nextafter(np.float32(box), np.float32(0)),) * 3, (np.float32(-0.0),) * 3]
        tpts = np.asarray(on, np.float32)
        rpts = np.concatenate([tpts + np.float32((1.7, -1.7, 1.0)), tpts + np.float32((-2.9, 0.0, 0.9))]).astype(np.float32)
        xyz = np.concatenate([tpts, rpts]).T.copy()
        T, R = np.arange(len(tpts), dtype=np.int32), np.arange(len(tpts), xyz.shape[1], dtype=np.int32)
        for rlo, rhi in ((0.0, rmax), (2.6, 3.037)):
            s = same_masks(lib, xyz, box, T, R, rlo, rhi, split=split, gpu=device, what=("boundaries", split, rhi))
            assert s.any()
            checked += 1
    return checked


def test_mask_exactness_on_the_emulator(emu_lib, oracle):
    assert mask_exactness(emu_lib, oracle) == len(TW.RADII) + 24 + 4


# ---- 3. the blob system: walk == all pairs == yardstick ---------------------------------------------------------------------------------------

def on_the_blob(lib, O, device=False):
    coords, topo, s, st, mass = blob_case(O, 4)
    shell = (s["blob"], 0.0, 3.5)
    props = [("shell", st, s["wo"], shell, 10.0), ("static", st, s["wo"], None, 10.0)]
    for cell in (dict(box=50.0), dict(box=(50.0, 50.0, 50.0), tilt=TILT), dict(box=50.0, flags=3)):
        tri = "tilt" in cell
        cc = coords[:1] if tri else coords            # (the yardstick's all-pairs arithmetic has no slab shortcut in a tilted cell)
        ykw = dict(tilt=cell.get("tilt", (0.0, 0.0, 0.0)), flags=cell.get("flags", 7))
        want, pops = S.shell_sdf(O, cc, cell["box"], st, mass, (s["wo"], shell), 10.0, **ykw)
        static, _ = S.shell_sdf(O, cc, cell["box"], st, mass, (s["wo"], None), 10.0, **ykw)
        if tri:
            assert 0 < pops[0] < s["wo"].size and want.sum() > 0 and (want <= static).all() and not np.array_equal(want, static)
        else:
            caps(want, pops, static, s["wo"].size)
        evs = both_paths(lib, props, cc, cell["box"], device=device, mass=mass, **{k: v for k, v in cell.items() if k != "box"})
        for ev in evs:
            check(ev, "shell", want, 10.0)
            check(ev, "static", static, 10.0)
    # a target list that names members of the structures: the exclusion rule by atom identity, with and without spec_sdf_include_self
    T = np.concatenate([s["blob"][:60], s["wo"]]).astype(np.int32)
    for inc in (0, 1):
        old = O.set_spec("sdf_include_self", inc)
        try:
            want, pops = S.shell_sdf(O, coords, 50.0, st, mass, (T, (s["h"], 1.2, 1.8)), 10.0)
            static, _ = S.shell_sdf(O, coords, 50.0, st, mass, (T, None), 10.0)
            caps(want, pops, static, T.size)
            with options(lib, spec_sdf_include_self=inc):
                evs = both_paths(lib, [("shell", st, T, (s["h"], 1.2, 1.8), 10.0)], coords, 50.0, device=device, mass=mass)
        finally:
            O.set_spec("sdf_include_self", old)
        for ev in evs:
            check(ev, "shell", want, 10.0)
    # spec_within_exclude_ref: T minus R, formed by the evaluator; the atoms of T in R never take part
    T = np.concatenate([s["wo"], s["h"][:500]]).astype(np.int32)
    want, pops = S.shell_sdf(O, coords, 50.0, st, mass, (T, (s["h"], 1.2, 1.8)), 10.0, exclude_ref=True)
    static, _ = S.shell_sdf(O, coords, 50.0, st, mass, (T, None), 10.0)
    kept, _ = S.shell_sdf(O, coords, 50.0, st, mass, (T, (s["h"], 1.2, 1.8)), 10.0)
    caps(want, pops, static, T.size)                  # (populations against |T|: T minus R is smaller still)
    assert (want <= kept).all() and not np.array_equal(want, kept)         # the hydrogens of T are members when they stay: the switch shows
    with options(lib, spec_within_exclude_ref=1):
        evs = both_paths(lib, [("shell", st, T, (s["h"], 1.2, 1.8), 10.0)], coords, 50.0, device=device, mass=mass)
    for ev in evs:
        check(ev, "shell", want, 10.0)


def test_walk_brute_and_yardstick_on_the_blob_system(emu_lib, oracle):
    on_the_blob(emu_lib, oracle)


def mask_rule(lib, O, device=False):
    """which path a shell gets by itself: all pairs for a reference list below shell_brute_below atoms (480), the walk from
    there on where a grid exists; the option moves the line, 0 removes it.  Same volume either way."""
    coords, topo, s, st, mass = blob_case(O, 2)
    vols = []
    for nr, below, walk in ((479, None, False), (480, None, True), (2000, None, True), (30, None, False), (30, 0, True), (30, 30, True),
                            (2000, 2001, False)):
        props = [("v", st, s["wo"], (s["blob"][:nr], 0.0, 3.5), 10.0)]
        ev, n = profiled(lib, lambda: run(lib, props, coords, 50.0, device=device, mass=mass), **({} if below is None else dict(shell_brute_below=below)))
        assert (n["shell_mask"] >= 1 and n["shell_mask_brute"] == 0) if walk else (n["shell_mask_brute"] >= 1 and n["shell_mask"] == 0), (nr, below, n)
        assert n["sdf_scatter"] >= 1
        vols.append(((nr, walk), vol(ev, "v")))
    assert lib.vmd_set_option(b"shell_brute_below", 480) == 480           # the default, and every override above was undone
    by_nr = {}
    for (nr, walk), v in vols:
        by_nr.setdefault(nr, []).append((walk, v))
    for nr in (30, 2000):
        assert {w for w, _ in by_nr[nr]} == {False, True} and all(np.array_equal(v, by_nr[nr][0][1]) for _, v in by_nr[nr]) and by_nr[nr][0][1].sum() > 0


def test_the_rule_between_walk_and_all_pairs(emu_lib, oracle):
    mask_rule(emu_lib, oracle)


# ---- 4. identities that need no yardstick -------------------------------------------------------------------------------------------------------

IDENTITY_SCRIPT = ("s1 = resname(\"ALA\")[2:8];"
                   "v = sdf(s1, water and element('O') and within(3.5, not water), 10.0);"
                   "nw = count(water and element('O') and within(3.5, not water));"
                   "g = rdf(water and element('O') and within(3.5, not water), element('H'), 1.0:6.0);"
                   "all_in = sdf(s1, water and element('O') and within(0.0:2.0, water and element('O')), 10.0);"
                   "static = sdf(s1, water and element('O'), 10.0);")


def identities(lib, O, device=False, F=6):
    import cases
    coords, topo = TG.blob_system(O, n_atoms=3000, n_blob=200, F=F)
    ir, info = script.compile_script(IDENTITY_SCRIPT, topo, lib=lib, within=True, shell_rdf=True, shell_sdf=True)
    mass = np.asarray(topo.mass, np.float32)
    ev = evaluate(lib, ir, coords, 30.0, device=device, mass=mass)
    # a shell that contains all of T (every atom is within 0 of itself) gives the static sdf's volume
    assert np.array_equal(vol(ev, "all_in"), vol(ev, "static")) and vol(ev, "static").sum() > 0
    assert TG.bits_equal(ev.property_data("all_in").values, ev.property_data("static").values)
    assert vol(ev, "v").sum() > 0 and (vol(ev, "v") <= vol(ev, "static")).all() and not np.array_equal(vol(ev, "v"), vol(ev, "static"))
    # the mask of frame f is what count() reports for it, and what the rdf over the same shell used (its weights are the populations)
    cell = V.make_unitcell(30.0)
    sysm, traj = V.MolSystem(coords.shape[2], mass=mass, unitcell=cell), cases.make_traj(lib, coords, cell, device)
    nw = TG.rows(ev, "nw")[:, 0]
    assert len(set(nw.tolist())) > 1 and (nw > 0).all()
    masks = [ev.shell_mask("v", sysm, traj, f) for f in range(F)]
    for f in range(F):
        assert int(masks[f].sum()) == int(nw[f])
        assert np.array_equal(masks[f], ev.shell_mask("nw", sysm, traj, f)) and np.array_equal(masks[f], ev.shell_mask("g", sysm, traj, f, which=0))
        assert not masks[f][np.setdiff1d(np.arange(coords.shape[2]), info["v"]["target"])].any()
    # the populations an rdf used show only in its fp64 weights (SPEC S4: N_ref = |H(f)|).  Frame by frame, the rdf over the shell is then
    # the STATIC rdf whose reference list is the mask's atoms, through the same library: the same host arithmetic on the same population,
    # so weights and counts are equal to the bit - a population off by one would change every weight
    for f in range(F):
        q = V.ScriptIR(lib)
        q.add_rdf("h", np.nonzero(masks[f])[0].astype(np.int32), info["g"]["target"], (1.0, 6.0))
        one_s = evaluate_range(lib, q, coords, 30.0, [(f, f + 1)], device, mass).property_data("h")
        one_g = evaluate_range(lib, ir, coords, 30.0, [(f, f + 1)], device, mass).property_data("g")
        w_s, w_g = np.asarray(one_s.weights64), np.asarray(one_g.weights64)
        assert np.array_equal(w_s.view(np.int64), w_g.view(np.int64)) and (w_g > 0).all(), f
        assert np.array_equal(one_s.counts, one_g.counts) and np.asarray(one_g.counts).sum() > 0, f
    # frames [a, b) == the sum of the single-frame evaluations == the sum of STATIC sdfs with target = H(f), frame by frame
    a, b = 1, 5
    part = evaluate_range(lib, ir, coords, 30.0, [(a, b)], device, mass)
    singles = np.zeros_like(vol(part, "v"))
    statics = np.zeros_like(singles)
    for f in range(a, b):
        singles += vol(evaluate_range(lib, ir, coords, 30.0, [(f, f + 1)], device, mass), "v")
        q = V.ScriptIR(lib)
        q.add_sdf("h", info["v"]["structures"], np.nonzero(masks[f])[0].astype(np.int32), 10.0)
        statics += vol(evaluate_range(lib, q, coords, 30.0, [(f, f + 1)], device, mass), "h")
    assert np.array_equal(vol(part, "v"), singles) and np.array_equal(singles, statics) and singles.sum() > 0
    assert not np.array_equal(vol(part, "v"), vol(ev, "v"))


def evaluate_range(lib, ir, coords, box, ranges, device, mass):
    """evaluate() without its all-frames assertion: a sub-range of the trajectory (the reference pose stays trajectory frame 0's)"""
    import cases
    F, _, N = coords.shape
    cell = V.make_unitcell(box)
    ev = V.ScriptEval(F, ir)
    sysm, traj = V.MolSystem(N, mass=mass, unitcell=cell), cases.make_traj(lib, coords, cell, device)
    for beg, end in ranges:
        assert ev.frame_range(sysm, traj, beg, end)
    return ev


def test_identities(emu_lib, oracle):
    identities(emu_lib, oracle)


# ---- 5. call patterns ------------------------------------------------------------------------------------------------------------------------------

CALL_SCRIPT = ("s1 = resname(\"ALA\")[2:8]; v = sdf(s1, water and element('O') and within(3.5, not water), 10.0);"
               "w = sdf(s1, element('H') and within(1.0:4.0, resname(\"ALA\")), 8.0); d = distance(10, 30);"
               "g = rdf(water and element('O') and within(3.5, not water), element('O'), 6.0);")
CALL_NAMES = ("v", "w")
RAGGED = [(0, 7), (7, 8), (8, 21), (21, 30)]


def same_vol(ev, ref, names=CALL_NAMES, what=""):
    for name in names:
        assert np.array_equal(vol(ev, name), vol(ref, name)), (what, name)
        assert vol(ref, name).sum() > 0


def call_patterns(lib, O, device=False):
    """on the walk, whatever |R| is: the path with state between batches (cell builds, bucket capacities, the overflow flag)"""
    with options(lib, shell_brute_below=0):
        _call_patterns(lib, O, device)


def _call_patterns(lib, O, device):
    import cases
    coords, topo = TG.blob_system(O, n_atoms=3000, n_blob=200, F=30)
    mass = np.asarray(topo.mass, np.float32)
    ir, info = script.compile_script(CALL_SCRIPT, topo, lib=lib, shell_rdf=True, shell_sdf=True)
    runit = lambda **kw: evaluate(lib, ir, coords, 30.0, device=device, mass=mass, **kw)
    one_call = runit()
    i = info["v"]
    sh = i["target_shell"]
    want, pops = S.shell_sdf(O, coords, 30.0, i["structures"], mass, (i["target"], (sh["ref"], sh["rmin"], sh["rmax"])), 10.0)
    static, _ = S.shell_sdf(O, coords, 30.0, i["structures"], mass, (i["target"], None), 10.0)
    caps(want, pops, static, len(i["target"]))
    check(one_call, "v", want, 10.0)
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
    with options(lib, shell_brute_below=480):         # |R| = 200 and 70: all pairs by the rule
        got["the rule's own choice"] = runit()
        got["the rule's own choice, pooled"] = runit(pooled=(4, 4))
    for ilp in (8, 16):
        old = lib.vmd_hip_set_sdf_ilp(ilp)
        try:
            got[f"ilp {ilp}"] = runit()
        finally:
            lib.vmd_hip_set_sdf_ilp(old)
    if lib.vmd_device_count() > 0:
        got["resident" if not device else "host"] = evaluate(lib, ir, coords, 30.0, device=not device, mass=mass)
    # block partials, and a second eval served from them over a sub-range (filtered evaluation)
    full = V.ScriptEval(30, ir); full.set_block_frames(5)
    cell = V.make_unitcell(30.0)
    sysm, traj = V.MolSystem(coords.shape[2], mass=mass, unitcell=cell), cases.make_traj(lib, coords, cell, device)
    assert full.frame_range(sysm, traj, 0, 30)
    got["block partials"] = full
    for what, ev in got.items():
        same_vol(ev, one_call, what=what)
    filt = V.ScriptEval(30, ir); filt.set_source(full)
    assert filt.frame_range(sysm, traj, 5, 22)
    assert filt.frame_stats()[1] > 0
    direct = V.ScriptEval(30, ir)
    assert direct.frame_range(sysm, traj, 5, 22)
    same_vol(filt, direct, what="filtered from block partials")
    assert not np.array_equal(vol(direct, "v"), vol(one_call, "v"))
    ahead = V.ScriptEval(30, ir); ahead.set_block_frames(5)
    assert ahead.frame_range_pooled(sysm, traj, 0, 30, 8, 1)
    same_vol(ahead, one_call, what="pooled with block partials")
    # clear_data, then the same range again: the volume starts from zero
    again = V.ScriptEval(30, ir)
    assert again.frame_range(sysm, traj, 0, 30)
    again.clear_data()
    assert not again.frame_mask().any()
    assert again.frame_range(sysm, traj, 0, 30)
    same_vol(again, one_call, what="clear_data + re-evaluation")
    # a shell radius above half the cell: no grid for that shell alone, the other one keeps the walk
    o = np.nonzero(np.asarray(topo.elements) == "O")[0].astype(np.int32)
    blob = np.arange(200, dtype=np.int32)
    props = [("wide", i["structures"], o, (blob, 0.0, 16.0), 10.0), ("near", i["structures"], o, (blob, 0.0, 3.5), 10.0)]
    ev, n = profiled(lib, lambda: run(lib, props, coords[:2], 30.0, device=device, mass=mass))
    assert n["shell_mask"] >= 1 and n["shell_mask_brute"] >= 1, n
    for name, st_, t_, sh_, cut in props:
        check(ev, name, S.shell_sdf(O, coords[:2], 30.0, st_, mass, (t_, sh_), cut)[0], cut)


def test_call_patterns(emu_lib, oracle):
    call_patterns(emu_lib, oracle)


# ---- 6. a pencil-bucket overflow ---------------------------------------------------------------------------------------------------------------------

def overflow_case(lib, O, device=False):
    """the construction of test_shell_rdf.overflow_case: the middle frames pile every oxygen into one pencil, a bucket of the cell build of
    R sized from the batch's ends overflows, and the batch - cell build, walk and masked scatter - is repeated.  The volume equals the
    yardstick's: no voxel was counted twice."""
    import cases
    n, box, F = 3000, 60.0, 12
    coords = cases.water_box(O, 5, n, box, F)
    o, h = cases.oxygen(n), cases.hydrogen(n)
    rng = np.random.default_rng(3)
    for f in (5, 6, 7):
        coords[f][:, o] = rng.uniform(1.0, 11.0, (3, o.size)).astype(np.float32)
    st = np.stack([np.arange(3 * k, 3 * k + 3) for k in (10, 400)]).astype(np.int32)       # two waters as the structures
    mass = np.tile(np.float32([15.999, 1.008, 1.008]), n // 3)
    T = h
    shell = (o, 0.5, 1.2)                    # R = every oxygen: the selection whose buckets overflow; a hydrogen is in when it is bonded
    want, pops = S.shell_sdf(O, coords, box, st, mass, (T, shell), 12.0)
    static, _ = S.shell_sdf(O, coords, box, st, mass, (T, None), 12.0)
    caps(want, pops, static, T.size)
    with options(lib, cells_small=0, cells_cap_sample=2):
        for bf, defer in ((0, 1), (4, 1), (4, 0)):
            with options(lib, batch_frames=bf, defer_sync=defer):
                ev = run(lib, [("v", st, T, shell, 12.0), ("s", st, T, None, 12.0)], coords, box, device=device, mass=mass)
                assert ev.cell_build_stats()[0] >= 1, (bf, defer)
                check(ev, "v", want, 12.0)
                check(ev, "s", static, 12.0)


def test_a_bucket_overflow_repeats_the_batch_and_counts_once(emu_lib, oracle):
    overflow_case(emu_lib, oracle)


# ---- 7. co-evaluation, multi-rank ------------------------------------------------------------------------------------------------------------------------

STATIC_SCRIPT = ("s1 = resname(\"ALA\")[2:8]; goo = rdf(element('O'), element('O'), 8.0); v = sdf(s1, element('H'), 10.0);"
                 "nw = count(water and element('O') and within(3.5, not water)); d = distance(10, 30);")
SHELL_LINE = "vs = sdf(s1, water and element('O') and within(3.5, not water), 10.0);"


def coevaluation(lib, O, device=False):
    coords, topo = TG.blob_system(O, n_atoms=3000, n_blob=200, F=4)
    mass = np.asarray(topo.mass, np.float32)
    ev0 = evaluate(lib, script.compile_script(STATIC_SCRIPT, topo, lib=lib, within=True)[0], coords, 30.0, device=device, mass=mass)
    ir1, info = script.compile_script(STATIC_SCRIPT + SHELL_LINE, topo, lib=lib, within=True, shell_sdf=True)
    ev1 = evaluate(lib, ir1, coords, 30.0, device=device, mass=mass)
    for name in ("goo", "v", "nw", "d"):
        a, b = ev0.property_data(name), ev1.property_data(name)
        assert TG.bits_equal(a.values, b.values) and np.asarray(a.values).any(), name
        if a.counts is not None:
            assert np.array_equal(a.counts, b.counts), name
    assert np.array_equal(np.asarray(ev0.property_data("goo").weights64).view(np.int64), np.asarray(ev1.property_data("goo").weights64).view(np.int64))
    i = info["vs"]
    sh = i["target_shell"]
    want, pops = S.shell_sdf(O, coords, 30.0, i["structures"], mass, (i["target"], (sh["ref"], sh["rmin"], sh["rmax"])), 10.0)
    varied(pops, len(i["target"]))
    check(ev1, "vs", want, 10.0)
    assert np.array_equal(TG.rows(ev1, "nw")[:, 0], pops.astype(np.float32))


def test_static_properties_are_unchanged_by_a_shell_sdf_line(emu_lib, oracle):
    coevaluation(emu_lib, oracle)


MERGE_SCRIPT = "s1 = resname(\"ALA\")[2:8]; v = sdf(s1, water and element('O') and within(3.5, not water), 10.0); d = distance(10, 30);"


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
    ir = script.compile_script(MERGE_SCRIPT, topo, lib=lib, shell_sdf=True)[0]
    F = coords.shape[0]
    ev = V.ScriptEval(F, ir)
    beg, end = shard_frames(F, rank, world)
    cell = V.make_unitcell(30.0)
    assert ev.frame_range(V.MolSystem(coords.shape[2], unitcell=cell), V.HostTrajectory(coords, cell), beg, end)
    reduce_eval(ev)
    assert ev.frame_mask().all()
    pd = ev.property_data("v")
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), counts=np.asarray(pd.counts), values=np.asarray(pd.values))
    dist.destroy_process_group()


def test_two_rank_merge_equals_the_single_evaluation(emu_lib, oracle, tmp_path):
    import torch.multiprocessing as mp
    port = 43500 + (os.getpid() % 2000)
    mp.spawn(_merge_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    coords, topo = TG.blob_system(oracle, n_atoms=3000, F=7)
    ir = script.compile_script(MERGE_SCRIPT, topo, lib=emu_lib, shell_sdf=True)[0]
    pd = evaluate(emu_lib, ir, coords, 30.0).property_data("v")
    assert np.asarray(pd.counts).sum() > 0
    for r in range(2):
        z = np.load(tmp_path / f"rank{r}.npz")
        assert np.array_equal(z["counts"], pd.counts) and TG.bits_equal(z["values"], pd.values)


# ---- 8. front-end --------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def topo():
    return synth.water_box_topology(200 + 933 * 3, n_blob=200)


OPT_INS = dict(angles=True, shape=True, rmsd=True, within=True, shell_rdf=True)


def test_without_the_opt_in_nothing_changes(host_lib, topo):
    import test_rmsd
    assert test_rmsd._old_ir(host_lib).fingerprint() == test_rmsd.PARENT_FINGERPRINT          # the literal the parent's suite holds
    text = VIAMD_DEFAULT_SCRIPT + TW.NW_LINE + TR.GS_LINE.replace("gs =", "gr =") + GS_LINE
    ir_a, rep_a = script.compile_script_native(text, topo, lib=host_lib, partial=True, **OPT_INS)
    ir_b, rep_b = script.compile_script_native(text, topo, lib=host_lib, partial=True, shell_sdf=False, **OPT_INS)
    ir_py, _, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, shell_sdf=False, **OPT_INS)
    assert ir_a.property_names() == ir_b.property_names() == ir_py.property_names() == ["d1", "a1", "r", "v", "lin", "plan", "iso", "nw", "gr"]
    assert ir_a.fingerprint() == ir_b.fingerprint() == ir_py.fingerprint() and rep_a == rep_b == rep_py
    k = rep_a["skipped"][0]
    assert [s["names"] for s in rep_a["skipped"]] == ["gs"] and text[k["beg"]:k["end"]] == GS_LINE[1:-1]
    assert k["reason"] == "unsupported function 'within' (outside the rdf / sdf / distance path)"      # the parent commit's words
    assert GS_LINE[1:] in rep_a["fallback_source"]
    # scripts without the form keep their fingerprints and reports whatever the new bit says
    for text0, kw in ((VIAMD_DEFAULT_SCRIPT, OPT_INS), (VIAMD_DEFAULT_SCRIPT, {}), (VIAMD_DEFAULT_SCRIPT + TW.NW_LINE + TR.GS_LINE, OPT_INS),
                      ("x = within(3, all); g = rdf(all, within(3, all), 5.0); v = sdf(resname(\"ALA\"), element('O'), 5.0); d = distance(within(2, all), 2);", {})):
        res = [script.compile_script_native(text0, topo, lib=host_lib, partial=True, shell_sdf=w, **kw) for w in (False, True)]
        res.append(script.compile_script(text0, topo, lib=host_lib, partial=True, shell_sdf=True, **kw)[::2])
        assert len({r[0].fingerprint() for r in res}) == 1 and res[0][1] == res[1][1] == res[2][1], text0
    # a static sdf compiled with the bit is the ir vmd_ir_add_sdf builds
    st = np.arange(200, dtype=np.int32).reshape(20, 10)
    o = np.nonzero(np.asarray(topo.elements) == "O")[0]
    q = V.ScriptIR(host_lib); q.add_sdf("v", st, o, 5.0)
    q2 = V.ScriptIR(host_lib); q2.add_sdf_shell("v", st, o, 5.0)
    assert q.fingerprint() == q2.fingerprint() == script.compile_script_native("v = sdf(resname(\"ALA\"), element('O'), 5.0);", topo, lib=host_lib, shell_sdf=True).fingerprint()
    for compiler in (script.compile_script_native, script.compile_script):
        with pytest.raises(script.ScriptError) as err:
            compiler("s1 = resname(\"ALA\")[2:8];" + GS_LINE[1:], topo, lib=host_lib, **OPT_INS)
        assert str(err.value) == "unsupported function 'within' (outside the rdf / sdf / distance path)"


def test_default_script_with_the_shell_sdf_line(host_lib, topo):
    text = VIAMD_DEFAULT_SCRIPT + GS_LINE
    ir_c, rep_c = script.compile_script_native(text, topo, lib=host_lib, partial=True, **ALL_BITS)
    ir_py, info, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, **ALL_BITS)
    assert ir_c.property_names() == ir_py.property_names() == ["d1", "a1", "r", "v", "lin", "plan", "iso", "gs"]
    assert ir_c.fingerprint() == ir_py.fingerprint() and ir_c.property_flags("gs") == ir_c.property_flags("v")
    assert rep_c == rep_py and rep_c["skipped"] == []
    fb = rep_c["fallback_source"]
    assert len(fb) == len(text) and fb.strip() == 's1 = resname("ALA")[2:8];'
    i = info["gs"]
    assert i["kind"] == "sdf" and i["cutoff"] == 10.0 and i["structures"].shape == (7, 10) and len(i["target"]) == 20 + 933
    assert (i["target_shell"]["rmin"], i["target_shell"]["rmax"]) == (0.0, 3.5) and list(i["target_shell"]["ref"]) == list(range(200))
    assert np.array_equal(i["structures"], info["v"]["structures"])
    assert int(host_lib.vmd_ir_work_per_frame(ir_c.h)) - int(host_lib.vmd_ir_work_per_frame(
        script.compile_script_native(VIAMD_DEFAULT_SCRIPT, topo, lib=host_lib, angles=True, shape=True).h)) == 7 * (953 + 10) + 953 + 200
    strict = script.compile_script_native(text, topo, lib=host_lib, **ALL_BITS)
    assert strict.fingerprint() == ir_c.fingerprint()


# (statement, K, m, |T|, shell (|R|, a, b) or None)
ACCEPTED = [
    ("v = sdf(resname(\"ALA\"), within(3.5, resname(\"ALA\")), 5.0);", 20, 10, 2999, (200, 0.0, 3.5)),
    ("v = sdf(resname(\"ALA\")[2:8], within(3.5:5.0, protein) and water, 8.0);", 7, 10, 2799, (200, 3.5, 5.0)),
    ("v = sdf(resname(\"ALA\"), water and within(2, atom(1:30)) and element('O'), 6.0);", 20, 10, 933, (30, 0.0, 2.0)),
    ("v = sdf(resname(\"ALA\"), (element('O') or element('N')) and not water and within(1.5, (water)), 4.0);", 20, 10, 40, (2799, 0.0, 1.5)),
    ("s = resname(\"ALA\")[2:8]; w = water and element('O'); v = sdf(s, w and within(0.5:2.5, s), 7.0);", 7, 10, 933, (70, 0.5, 2.5)),
    ("v = sdf(resname(\"ALA\"), element('O'), 5.0);", 20, 10, 953, None),
]

SKIPPED = [
    ("v = sdf(resname(\"ALA\"), water and not within(3, protein), 5.0);", "within() must be a factor of the top-level AND"),
    ("v = sdf(resname(\"ALA\"), water or within(3, protein), 5.0);", "within() must be a factor of the top-level AND"),
    ("v = sdf(resname(\"ALA\"), water and (within(3, protein)), 5.0);", "within() must be a factor of the top-level AND"),
    ("v = sdf(resname(\"ALA\"), within(3, protein) and within(5, water), 5.0);", "an sdf argument takes exactly one within() factor, found 2"),
    ("v = sdf(resname(\"ALA\"), water and within(3, within(4, protein)), 5.0);", "an sdf argument takes exactly one within() factor, found 2"),
    ("v = sdf(resname(\"ALA\") and within(3, water), water, 5.0);", "within() in the structures argument of sdf() is not supported"),
    ("v = sdf(within(3, water), water and within(3, protein), 5.0);", "within() in the structures argument of sdf() is not supported"),
    ("v = distance(within(3, protein), water);", "unsupported function 'within'"),
    ("v = distance_min(water, within(3, protein));", "unsupported function 'within'"),
    ("v = sdf(resname(\"ALA\"), resname(\"XYZ\") and within(3, protein), 5.0);", "v: empty selection"),
    ("v = sdf(resname(\"ALA\"), water and within(3, resname(\"XYZ\")), 5.0);", "v: empty selection"),
    ("v = sdf(resname(\"ALA\"), water and within(0, protein), 5.0);", "within needs a radius > 0"),
    ("v = sdf(resname(\"ALA\"), water and within(5:3, protein), 5.0);", "within range needs 0 <= a < b"),
    ("v = sdf(resname(\"ALA\"), water and within(3:3, protein), 5.0);", "within range needs 0 <= a < b"),
    ("v = sdf(resname(\"ALA\"), water and within(3), 5.0);", "expected ,"),
    ("v = sdf(resname(\"ALA\"), water and within(protein, 3), 5.0);", "expected num"),
    ("d = sdf(resname(\"ALA\"), water and within(3, protein), 5.0);", "already defined"),
]


@pytest.mark.parametrize("stmt,K,m,nt,sh", ACCEPTED)
def test_accepted_forms(host_lib, topo, stmt, K, m, nt, sh):
    ir_c = script.compile_script_native(stmt, topo, lib=host_lib, shell_sdf=True)
    ir_py, info = script.compile_script(stmt, topo, lib=host_lib, shell_sdf=True)
    assert ir_c.property_names() == ir_py.property_names() == ["v"] and ir_c.fingerprint() == ir_py.fingerprint()
    i = info["v"]
    assert i["structures"].shape == (K, m) and len(i["target"]) == nt
    got = i.get("target_shell")
    assert (got is None) == (sh is None)
    work = K * (nt + m)
    if sh:
        assert (len(got["ref"]), got["rmin"], got["rmax"]) == sh
        work += nt + sh[0]
        # the statement without its within() factor is another ir
        q = V.ScriptIR(host_lib); q.add_sdf("v", i["structures"], i["target"], i["cutoff"])
        assert q.fingerprint() != ir_c.fingerprint()
    assert int(host_lib.vmd_ir_work_per_frame(ir_c.h)) == work
    assert ir_c.property_flags("v") == L.FLAG_VOLUME


@pytest.mark.parametrize("stmt,reason", SKIPPED)
def test_skipped_forms(host_lib, topo, stmt, reason):
    text = "d = distance(1, 2);\n" + stmt + "\ne = distance(3, 4);"
    for compiler in (script.compile_script_native, script.compile_script):
        with pytest.raises((script.ScriptError, V.VmdError)) as err:
            compiler(text, topo, lib=host_lib, shell_sdf=True)
        assert reason in str(err.value)
    ir_c, rep_c = script.compile_script_native(text, topo, lib=host_lib, partial=True, shell_sdf=True)
    ir_py, _, rep_py = script.compile_script(text, topo, lib=host_lib, partial=True, shell_sdf=True)
    assert ir_c.property_names() == ir_py.property_names() == ["d", "e"] and ir_c.fingerprint() == ir_py.fingerprint()
    assert rep_c == rep_py and len(rep_c["skipped"]) == 1
    k = rep_c["skipped"][0]
    assert k["names"] == stmt.split(" ")[0] and reason in k["reason"] and text[k["beg"]:k["end"]] == stmt[:-1]
    assert stmt in rep_c["fallback_source"] and "distance(3, 4)" not in rep_c["fallback_source"]


# ---- 9. ABI ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_ir_validation_errors(host_lib):
    lib = host_lib
    for sym in ("vmd_ir_add_sdf_shell", "vmd_eval_shell_mask", "vmd_hip_within_atoms", "vmd_hip_within_brute_atoms", "vmd_hip_sdf_scatter_masked"):
        assert hasattr(lib, sym), sym
    ir = V.ScriptIR(lib)
    st = np.array([[0, 1], [2, 3]], np.int32)
    ok = ([1], 0.0, 3.0)
    for s_, t, cut, sh, msg in ((np.zeros((0, 2), np.int32), [1], 5.0, ok, "sdf reference structures is empty"), (st, [], 5.0, ok, "sdf target set is empty"),
                                (st, [0, -1], 5.0, ok, "negative"), (np.array([[0, -3]], np.int32), [1], 5.0, ok, "negative"),
                                (st, [1], 0.0, ok, "sdf cutoff must be positive"), (st, [1], 5.0, ([], 0.0, 3.0), "within reference set is empty"),
                                (st, [1], 5.0, ([-2], 0.0, 3.0), "negative"),
                                (st, [1], 5.0, ([1], 3.0, 3.0), "within range must be finite and satisfy 0 <= rmin < rmax"),
                                (st, [1], 5.0, ([1], -1.0, 3.0), "0 <= rmin < rmax"), (st, [1], 5.0, ([1], 0.0, float("inf")), "finite"),
                                (st, [1], 5.0, ([1], float("nan"), 3.0), "finite")):
        with pytest.raises(V.VmdError, match=msg):
            ir.add_sdf_shell("v", s_, t, cut, target_shell=sh)
    with pytest.raises(V.VmdError, match="name is empty"):
        ir.add_sdf_shell("", st, [1], 5.0, target_shell=ok)
    assert ir.property_count() == 0
    ir.add_distance("d", [0], [1])
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_sdf_shell("d", st, [1], 5.0, target_shell=ok)
    ir.add_sdf_shell("v", st, [1, 5, 7], 5.0, target_shell=([2, 3, 4, 5], 0.0, 2.0))
    assert ir.property_names() == ["d", "v"] and ir.property_flags("v") == L.FLAG_VOLUME
    assert int(lib.vmd_ir_work_per_frame(ir.h)) == 1 + 2 * (3 + 2) + (3 + 4)

    def fp(*args, **kw):
        q = V.ScriptIR(lib)
        q.add_sdf_shell(*args, **kw)
        return q.fingerprint()
    base = ("v", st, [3, 4], 6.0)
    sh = ([5, 6], 0.0, 2.0)
    fps = [fp(*base), fp(*base, target_shell=sh), fp(*base, target_shell=([5], 0.0, 2.0)), fp(*base, target_shell=([5, 6], 0.5, 2.0)),
           fp(*base, target_shell=([5, 6], 0.0, 2.5)), fp("h", *base[1:], target_shell=sh)]
    q = V.ScriptIR(lib); q.add_sdf(*base)
    assert fps[0] == q.fingerprint() and len(set(fps)) == len(fps)
    # an rdf whose target is the same shell is another ir: the kinds differ
    r = V.ScriptIR(lib); r.add_rdf_shell("v", [0, 1, 2, 3], [3, 4], 6.0, target_shell=sh)
    assert r.fingerprint() not in fps
    ir2 = V.ScriptIR(lib)
    ir2.add_sdf_shell("v", st, [1], 3.0, target_shell=([99], 0.0, 3.0))
    if lib.vmd_device_count() > 0:
        with pytest.raises(V.VmdError, match="references atom 99"):
            TG.evaluate(lib, ir2, np.zeros((1, 3, 10), np.float32), 10.0)


# ---- 10. vmd_eval_shell_mask ---------------------------------------------------------------------------------------------------------------------------------------

MASK_SCRIPT = ("s1 = resname(\"ALA\")[2:8]; v = sdf(s1, water and element('O') and within(3.5, not water), 10.0);"
               "nw = count(element('H') and within(1.0:4.0, resname(\"ALA\")));"
               "g = rdf(water and element('O') and within(0.5:2.9, element('O')), element('H') and within(4.0, not water), 1.0:5.0);"
               "gt = rdf(element('O'), element('H') and within(4.0, not water), 1.0:5.0); s = sdf(s1, element('O'), 10.0); d = distance(10, 30);")


def shell_mask_product(lib, O, device=False):
    import cases
    F = 5
    coords, topo = TG.blob_system(O, n_atoms=3000, n_blob=200, F=F)
    N = coords.shape[2]
    mass = np.asarray(topo.mass, np.float32)
    ir, info = script.compile_script(MASK_SCRIPT, topo, lib=lib, within=True, shell_rdf=True, shell_sdf=True)
    ev = evaluate(lib, ir, coords, 30.0, device=device, mass=mass)
    cell = V.make_unitcell(30.0)
    sysm, traj = V.MolSystem(N, mass=mass, unitcell=cell), cases.make_traj(lib, coords, cell, device)
    bx = Box((30.0, 30.0, 30.0, 0.0, 0.0, 0.0), 7)
    before = {n: (ev.property_data(n).fingerprint, np.asarray(ev.property_data(n).values).copy()) for n in ir.property_names()}
    mask_before = ev.frame_mask().copy()
    sides = [("v", 1, (info["v"]["target"], info["v"]["target_shell"])), ("nw", 1, (info["nw"]["target"], info["nw"])),
             ("g", 0, (info["g"]["ref"], info["g"]["ref_shell"])), ("g", 1, (info["g"]["target"], info["g"]["target_shell"])),
             ("gt", 1, (info["gt"]["target"], info["gt"]["target_shell"]))]
    for name, which, (t, sh) in sides:
        pops = []
        for f in range(F):
            want = S.atom_mask(coords[f], bx, (t, (sh["ref"], sh["rmin"], sh["rmax"])), N)
            got = ev.shell_mask(name, sysm, traj, f, which=which)
            assert got.dtype == bool and got.shape == (N,) and np.array_equal(got, want), (name, which, f)
            pops.append(int(want.sum()))
        varied(np.asarray(pops), len(t))
    # the walk an evaluation used agrees with it: the count property's rows
    assert np.array_equal(TG.rows(ev, "nw")[:, 0], np.float32([ev.shell_mask("nw", sysm, traj, f).sum() for f in range(F)]))
    # what is not a shell is an error, never a zero
    for name, which, msg in (("s", 1, "is not a within\\(\\) shell"), ("d", 1, "is not a within\\(\\) shell"), ("gt", 0, "reference side of 'gt' is not a within"),
                             ("nw", 0, "reference side of 'nw' is not a within"), ("v", 0, "reference side of 'v' is not a within"),
                             ("nope", 1, "unknown property"), ("v", 2, "which must be 0")):
        with pytest.raises(V.VmdError, match=msg):
            ev.shell_mask(name, sysm, traj, 0, which=which)
    with pytest.raises(V.VmdError, match="outside the trajectory"):
        ev.shell_mask("v", sysm, traj, F)
    # cap too small: the failure value, nothing written
    words = np.full((N + 63) // 64, 0x5a5a5a5a5a5a5a5a, np.uint64)
    sysp = C.byref(sysm.c)
    wp = words.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.vmd_eval_shell_mask(ev.h, b"v", 1, sysp, traj.interface(), 0, wp, words.size - 1) == L.SHELL_MASK_FAILED
    assert "words needed" in lib.last_error() and (words == 0x5a5a5a5a5a5a5a5a).all()
    got = lib.vmd_eval_shell_mask(ev.h, b"v", 1, sysp, traj.interface(), 0, wp, words.size)
    assert got == int(ev.shell_mask("v", sysm, traj, 0).sum()) and got != L.SHELL_MASK_FAILED
    # nothing the evaluation keeps was touched
    for n, (fpr, vals) in before.items():
        pd = ev.property_data(n)
        assert pd.fingerprint == fpr and TG.bits_equal(pd.values, vals), n
    assert np.array_equal(ev.frame_mask(), mask_before)
    # before any frame was evaluated, and with an empty T minus R
    fresh = V.ScriptEval(F, ir)
    assert np.array_equal(fresh.shell_mask("v", sysm, traj, 2), ev.shell_mask("v", sysm, traj, 2)) and not fresh.frame_mask().any()
    with options(lib, spec_within_exclude_ref=1):
        q = V.ScriptIR(lib); q.add_within_count("n", [5, 6], [5, 6, 7], 0.0, 3.0)
        e2 = V.ScriptEval(F, q)
    assert not e2.shell_mask("n", sysm, traj, 0).any()


def test_shell_mask(emu_lib, oracle):
    shell_mask_product(emu_lib, oracle)


# ---- 11. VIAMD's default script plus a shell sdf line through the shim ------------------------------------------------------------------------------------------------

def build_shim_shell_sdf():
    """tests/native/shim_default_script_shell_sdf.cpp linked against the product library"""
    return native_host.build_shim("shim_default_script_shell_sdf")


def test_shim_default_script_with_the_shell_sdf_line_on_the_emulator(emu_lib, tmp_path):
    import conftest
    exe = native_host.build_shim("shim_default_script_shell_sdf", conftest.build_emu(), tmp_path / "shim_shell_sdf_emu")
    native_host.run_ok([exe, "8"], "OK frames=8 properties=8 gs=gpu fallback_frame_range_calls=0")
    out = native_host.run_ok([exe, "8", "nobit"], "OK frames=8 properties=8 gs=fallback")
    assert "fallback_frame_range_calls=0" not in out.stdout, out.stdout
