"""Mean-squared displacement over lag times on the emulator build and in the host-only entry points.  The rule: the rows of
the position table equal the frame's floats bit for bit, and every u64 of vmd_eval_msd equals the NumPy restatement (tests/msd_ref.py)
EXACTLY, for every launch choice.  Scenarios: known answers computed by hand here (an atom at rest; one atom moving 0.75 A per frame
through the face of an 8 A cell, with the axis open, along the body diagonal; a step of exactly half a cell; two atoms walking apart);
the size edges on seeded lattice random walks (steps of 0.25 A: the fp32 arithmetic is exact, a disagreement is an indexing error) around
the kernel's tile - atoms, origin span, lag chunk -, windows, lags, strides, a window that does not start at frame 0, a cell that changes
from frame to frame; one sweep on non-lattice fp32 coordinates; the evaluator's call patterns; the statement next to the other forms; the
two-rank merge; and the host-only part.  The emulator runs one lane at a time: tests/test_msd_gpu.py runs the same scenario functions on
the device, where the concurrency of the 64-bit atomics is what is checked."""
import ctypes as C
import hashlib
import os
import struct
import sys

import numpy as np
import pytest

import viamd_amd as V
from viamd_amd import _lib as L
from viamd_amd import script
from viamd_amd.eval import diffusion_coefficient

import cases
import cluster_cases as CL
import msd_cases as MC
import msd_ref as R
import test_geometry as TG
import test_rmsd as TR
from test_hbond import Options
from test_rama import OPT_INS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pos"
Q = 1 << 20


def tile(lib):
    a, s, c = C.c_int(0), C.c_int(0), C.c_int(0)
    assert lib.vmd_hip_msd_tile(C.byref(a), C.byref(s), C.byref(c)) == 0
    return a.value, s.value, c.value


def unitcells(cells):
    return V.make_unitcell(cells[0], cells[2], cells[1]) if isinstance(cells, tuple) else [V.make_unitcell(b, f, t) for b, t, f in cells]


class Run:
    """one evaluation of the position table of `atoms` over a host trajectory (vmd_hosttraj_*); device=True: a resident one"""

    def __init__(self, lib, coords, cells, atoms, device="pinned", ranges=None, ir=None, name=NAME, blocks=0):
        F, _, N = coords.shape
        self.atoms = np.asarray(atoms, np.int32)
        self.name = name
        if ir is None:
            ir = V.ScriptIR(lib)
            ir.add_msd(name, self.atoms)
        uc = unitcells(cells)
        self.ev = V.ScriptEval(F, ir)
        if blocks:
            self.ev.set_block_frames(blocks)
        self.sysm = V.MolSystem(N, unitcell=uc if isinstance(cells, tuple) else uc[0])
        self.traj = cases.make_traj(lib, coords, uc, device)
        for beg, end in ([(0, F)] if ranges is None else ranges):
            assert self.ev.frame_range(self.sysm, self.traj, beg, end)

    def table(self):
        return self.ev.property_data(self.name).msd_table.copy()

    def sums(self, beg=0, end=None, max_lag=None, stride=1):
        return self.ev.msd(self.name, beg, end, max_lag, stride).sums


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def check_table(rn, coords, cells, frames=None):
    want = R.table(coords, cells, rn.atoms)
    got = rn.table()
    assert got.dtype == np.float32 and got.shape == want.shape
    if frames is not None:
        rest = np.setdiff1d(np.arange(coords.shape[0]), frames)
        assert not got[rest].any()
        want[rest] = 0
    assert np.array_equal(bits(got), bits(want))
    return want


def query(rn, rows, what, beg=0, end=None, max_lag=None, stride=1):
    """one query against the restatement of `rows`, exactly"""
    end = rows.shape[0] if end is None else end
    max_lag = end - beg - 1 if max_lag is None else max_lag
    want = R.msd(rows, rn.atoms.size, beg, end, max_lag, stride)
    res = rn.ev.msd(rn.name, beg, end, max_lag, stride)
    got = res.sums
    assert got.dtype == np.uint64 and got.shape == (max_lag + 1, 4), what
    assert np.array_equal(got, want), (what, beg, end, max_lag, stride, np.argwhere(got != want)[:4])
    assert res.frames_used == end - beg
    tau = np.arange(max_lag + 1)
    origins = np.array([len(range(0, end - beg - t, stride)) for t in tau])
    assert np.array_equal(got[:, 3], (origins * rn.atoms.size).astype(np.uint64)), what
    assert not got[0, :3].any(), what
    msd, per_axis, terms = res
    assert msd.dtype == np.float64 and np.array_equal(terms, got[:, 3].astype(np.float64))
    assert np.array_equal(per_axis, got[:, :3] / (float(Q) * got[:, 3:4])) and np.array_equal(msd, per_axis.sum(axis=1))
    return got


# ---- 1. known answers, computed by hand ------------------------------------------------------------------------------------------------------

def known_answers(lib, device="pinned"):
    F = 40
    tau = np.arange(F, dtype=np.uint64)
    origins = (F - tau)
    zero = np.zeros(F, np.uint64)

    def columns(coords, cells, atoms):
        rn = Run(lib, coords, cells, atoms, device)
        rows = check_table(rn, coords, cells)
        return query(rn, rows, "known answer")

    # an atom at rest: every sum is 0 and terms = origins
    got = columns(MC.mover(F, step=(0.0, 0.0, 0.0)), MC.CUBE8, [0])
    assert np.array_equal(got, np.stack([zero, zero, zero, origins], axis=1))
    # 0.75 A per frame along x in a cell of 8 A: 0.5 + 39 * 0.75 = 29.75, three faces crossed; (0.75 tau)^2 2^20 = 9 tau^2 2^16 exactly
    coords = MC.mover(F)
    assert (np.diff(coords[:, 0, 0]) < 0).sum() == 3 and coords[:, 0, 0].max() < 8.0
    sq = np.uint64(9 << 16) * tau * tau * origins
    got = columns(coords, MC.CUBE8, [0])
    assert np.array_equal(got, np.stack([sq, zero, zero, origins], axis=1))
    # the same atom with the x axis open: no unwrap, the folded coordinate is taken as it stands
    x = coords[:, 0, 0].astype(np.float64)
    folded = np.array([int(((x[t:] - x[:F - t]) ** 2).sum() * Q) if t else 0 for t in range(F)], np.uint64)
    got = columns(coords, MC.OPEN_X, [0])
    assert np.array_equal(got, np.stack([folded, zero, zero, origins], axis=1)) and not np.array_equal(folded, sq)
    # ... and an open axis that is never crossed gives the periodic answer
    got = columns(MC.mover(F, step=(0.125, 0.0, 0.0), cells=MC.OPEN_X), MC.OPEN_X, [0])
    assert np.array_equal(got[:, 0], np.uint64(1 << 14) * tau * tau * origins)
    # along the body diagonal: the three columns alike
    got = columns(MC.mover(F, step=(0.75, 0.75, 0.75), start=(0.5, 7.25, 4.0)), MC.CUBE8, [0])
    assert np.array_equal(got, np.stack([sq, sq, sq, origins], axis=1))
    # backwards through the face
    got = columns(MC.mover(F, step=(-0.75, 0.0, 0.0)), MC.CUBE8, [0])
    assert np.array_equal(got, np.stack([sq, zero, zero, origins], axis=1))
    # a step of exactly half a cell, forwards and backwards: SPEC S3's comparisons are strict, so neither is a crossing - the displacement is
    # the 4 A the frames show, and back to the start after two steps
    half = np.zeros((3, 3, 2), np.float32)
    half[:, 0, 0] = (1.0, 5.0, 1.0)
    half[:, 0, 1] = (5.0, 1.0, 5.0)
    got = columns(half, MC.CUBE8, [0, 1])
    assert got.tolist() == [[0, 0, 0, 6], [4 * 16 * Q, 0, 0, 4], [0, 0, 0, 2]]
    # ... and one lattice step beyond half a cell is a crossing: 4.25 A forwards is 3.75 A backwards
    past = half.copy()
    past[:, 0, 0] = (1.0, 5.25, 1.5)
    got = columns(past, MC.CUBE8, [0])
    assert got[:, 0].tolist() == [0, int((3.75 ** 2 + 3.75 ** 2) * Q), int(7.5 ** 2 * Q)]
    # two atoms walking apart along y, 0.5 A per frame each: column 3 counts both
    pos = np.zeros((F, 3, 2))
    pos[:, 1, 0] = 4.0 + 0.5 * np.arange(F)
    pos[:, 1, 1] = 4.0 - 0.5 * np.arange(F)
    got = columns(MC.wrapped(pos, MC.CUBE8), MC.CUBE8, [0, 1])
    assert np.array_equal(got, np.stack([zero, np.uint64(2 << 18) * tau * tau * origins, zero, 2 * origins], axis=1))
    # an atom at rest next to the mover, the list in another order than the atoms
    got = columns(MC.mover(F, extra=2), MC.CUBE8, [2, 0])
    assert np.array_equal(got, np.stack([sq, zero, zero, 2 * origins], axis=1))


def test_known_answers_on_the_emulator(emu_lib):
    known_answers(emu_lib)


# ---- 2. size edges against the restatement -----------------------------------------------------------------------------------------------------

def edge_sizes(lib):
    A, S, LC = tile(lib)
    assert (A, S, LC) == (8, 32, 256), "the size edges below are chosen around the kernel's tile: revisit them with it"
    # (3 S frames: the window in which lags 63, 64 and 65 all have several origins - in 2 S + 1 frames lag 65 has none and 64 one)
    return sorted({1, 63, 64, 65, A - 1, A, A + 1, 2 * A + 1}), sorted({2, S - 1, S, S + 1, 2 * S + 1, 3 * S})


def size_sweep(lib, device="pinned", breathing=False):
    """every n of the edges, one evaluation of 3 S + 3 frames each, then the windows x lags x strides x starts as queries"""
    ns, windows = edge_sizes(lib)
    F = max(windows) + 3
    cells = MC.breathing_cells(F, 3) if breathing else MC.CUBE8
    count, asked = 0, set()
    for n in ns:
        coords, atoms = MC.lattice_walk(n, F, seed=n, cells=cells, natoms=n + 5)
        rn = Run(lib, coords, cells, atoms, device)
        rows = check_table(rn, coords, cells)
        for W in windows:
            for beg in (0, 3):
                for lag in sorted({0, 1, 63, 64, 65, W - 1}):
                    if lag >= W:
                        continue
                    for stride in (1, 2, 7, W + 3):
                        query(rn, rows, f"n {n}", beg, beg + W, lag, stride)
                        count += 1
                        asked.add((W, lag))
    assert {(3 * 32, lag) for lag in (63, 64, 65)} <= asked and count == 1344
    print(f"size sweep ({'a cell per frame' if breathing else 'one cell'}): {count} queries equal to the restatement")


def test_size_edges_on_the_emulator(emu_lib):
    size_sweep(emu_lib)


def test_size_edges_with_a_cell_per_frame_on_the_emulator(emu_lib):
    size_sweep(emu_lib, breathing=True)


def lag_chunks(lib, device="pinned"):
    """windows longer than a block's lag chunk: lags on either side of it, the last lag of the window"""
    A, S, LC = tile(lib)
    F = LC + 2 * S + 5
    for n in (3, A + 1):
        coords, atoms = MC.lattice_walk(n, F, seed=40 + n)
        rn = Run(lib, coords, MC.CUBE8, atoms, device)
        rows = check_table(rn, coords, MC.CUBE8)
        for beg, end in ((0, F), (2, LC + 3)):
            for lag in sorted({LC - 1, LC, LC + 1, end - beg - 1}):
                if lag < end - beg:
                    for stride in (1, 7):
                        query(rn, rows, f"lag chunks, n {n}", beg, end, lag, stride)


def test_lag_chunks_on_the_emulator(emu_lib):
    lag_chunks(emu_lib)


def liquid(lib, device="pinned"):
    """non-lattice fp32 coordinates: here the stated order of operations is what makes equality hold"""
    coords, cells = MC.liquid_walk(130, 70, seed=8)
    atoms = np.arange(0, 130, 2, dtype=np.int32)
    rn = Run(lib, coords, cells, atoms, device)
    rows = check_table(rn, coords, cells)
    assert np.abs(R.unwrap(rows, atoms.size)).max() >= 1, "nobody crossed a face"
    got = query(rn, rows, "liquid")
    assert got[1:, :3].all()
    for beg, end, lag, stride in ((0, 70, 40, 3), (5, 60, 54, 1), (11, 44, 7, 2)):
        query(rn, rows, "liquid", beg, end, lag, stride)


def test_non_lattice_coordinates_on_the_emulator(emu_lib):
    liquid(emu_lib)


def many_blocks(lib, device="pinned"):
    """n = 5 000, 64 frames, max_lag 63: 625 atom tiles x 2 spans of blocks add to the same 64 lag rows"""
    coords, atoms = MC.lattice_walk(5000, 64, seed=77)
    rn = Run(lib, coords, MC.CUBE8, atoms, device)
    rows = check_table(rn, coords, MC.CUBE8)
    query(rn, rows, "many blocks", 0, 64, 63, 1)


def dead_edge(lib, device="pinned"):
    """a frame whose x edge is not positive although the flag is set, in the middle of a batch that a good frame leads, and leading a batch
    of its own: its row holds L = 1 / L = 0 either way (the frame's own edge decides, not the batch's first frame), no count moves into
    it, and the query equals the restatement"""
    F, n = 6, 11
    cells = [MC.CUBE8] * F
    cells[3] = ((0.0, 8.0, 8.0), (0.0, 0.0, 0.0), 7)
    coords, atoms = MC.lattice_walk(n, F, seed=31, natoms=14)
    want = R.table(coords, cells, atoms)
    assert not want[3, 3 * n] and not want[3, 3 * n + 3] and want[3, 3 * n + 1] == 8.0 and want[2, 3 * n] == 8.0
    one = None
    for bf in (0, 1, 3):
        with Options(lib, batch_frames=bf):
            rn = Run(lib, coords, cells, atoms, device)
        rows = check_table(rn, coords, cells)
        got = query(rn, rows, f"a dead edge, batch_frames {bf}")
        one = got if one is None else one
        assert np.array_equal(got, one)


def test_a_frame_with_a_dead_edge_on_the_emulator(emu_lib):
    dead_edge(emu_lib)
    dead_edge(emu_lib, device=False)


def test_many_blocks_on_the_emulator(emu_lib):
    many_blocks(emu_lib)


# ---- 3. the evaluator ---------------------------------------------------------------------------------------------------------------------------

def call_patterns(lib, device="pinned"):
    """batch sizes, one call / two calls / two calls in reverse order, frame blocks, a partial range and its refusal, the query before and
    after an unrelated frame_range call, clear_data"""
    F, n = 12, 20
    cells = MC.breathing_cells(F, 5)
    coords, atoms = MC.lattice_walk(n, F, seed=21, cells=cells, natoms=31)
    first = Run(lib, coords, cells, atoms, device)
    rows = check_table(first, coords, cells)
    one = query(first, rows, "one call")
    part = query(first, rows, "a window", 3, 11, 5, 2)
    for kw in (dict(ranges=[(0, 7), (7, F)]), dict(ranges=[(7, F), (0, 7)]), dict(ranges=[(f, f + 1) for f in (5, 2, 9, 0, 11, 7, 1, 3, 10, 4, 8, 6)]),
               dict(blocks=2), dict(blocks=5, ranges=[(5, 10), (0, 5), (10, F)])):
        for bf in (0, 1, 2):
            with Options(lib, batch_frames=bf):
                rn = Run(lib, coords, cells, atoms, device, **kw)
            assert np.array_equal(bits(rn.table()), bits(rows)), (kw, bf)
            assert np.array_equal(rn.sums(), one) and np.array_equal(rn.sums(3, 11, 5, 2), part), (kw, bf)
    # a frame evaluated twice gets the same row twice; the query touches nothing the evaluator keeps
    assert first.ev.frame_range(first.sysm, first.traj, 2, 6)
    assert np.array_equal(bits(first.table()), bits(rows)) and np.array_equal(first.sums(), one)
    # frames 4 .. 8 alone: the rows of the others are zero, a window inside answers, one that reaches outside names the first missing frame
    some = Run(lib, coords, cells, atoms, device, ranges=[(4, 9)])
    check_table(some, coords, cells, frames=np.arange(4, 9))
    assert np.array_equal(some.sums(4, 9, 4, 1), R.msd(rows, n, 4, 9, 4, 1))
    for beg, end, miss in ((3, 9, 3), (4, 10, 9), (0, F, 0), (9, F, 9)):
        with pytest.raises(V.VmdError, match=f"frame {miss} of the window has not been evaluated"):
            some.sums(beg, end, 0)
    assert some.ev.frame_range(some.sysm, some.traj, 0, 4)              # an unrelated range: the answer stays, the window may grow
    assert np.array_equal(some.sums(4, 9, 4, 1), R.msd(rows, n, 4, 9, 4, 1)) and np.array_equal(some.sums(0, 9, 8, 1), R.msd(rows, n, 0, 9, 8, 1))
    # clear_data zeroes the table on the host and on the device, as it zeroes the angle table, and every frame counts as not evaluated
    some.ev.clear_data()
    assert not some.table().any()
    with pytest.raises(V.VmdError, match="frame 4 of the window has not been evaluated"):
        some.sums(4, 9, 0)
    assert some.ev.frame_range(some.sysm, some.traj, 0, F)
    assert np.array_equal(bits(some.table()), bits(rows)) and np.array_equal(some.sums(), one)


def test_call_patterns_on_the_emulator(emu_lib):
    call_patterns(emu_lib)
    call_patterns(emu_lib, device=False)


def overflow_case(lib, O, device="pinned"):
    """test_clusters.overflow_case's construction: the middle frames pile every oxygen into one pencil, a bucket sized from the batch's ends
    overflows and the batch is repeated.  The table's rows are written outside the overflow flag, twice the same."""
    n, box, F = 3000, 60.0, 12
    coords = cases.water_box(O, 5, n, box, F)
    o = cases.oxygen(n)
    rng = np.random.default_rng(3)
    for f in (5, 6, 7):
        coords[f][:, o] = rng.uniform(1.0, 11.0, (3, o.size)).astype(np.float32)
    atoms = o[:300].astype(np.int32)
    cells = ((box, box, box), (0.0, 0.0, 0.0), 7)
    rows = R.table(coords, cells, atoms)
    want = R.msd(rows, atoms.size, 0, F, F - 1)
    with Options(lib, cells_small=0, cells_cap_sample=2):
        for bf in (0, 4):
            with Options(lib, batch_frames=bf):
                ir = V.ScriptIR(lib)
                ir.add_msd(NAME, atoms)
                ir.add_rdf("goo", o, o, (0.0, 12.0))
                lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
                try:
                    rn = Run(lib, coords, cells, atoms, device, ir=ir)
                finally:
                    lib.vmd_profile_enable(False)
                nb = C.c_uint64(0)
                lib.vmd_profile_ms(b"cells_build", C.byref(nb))
                assert nb.value > ((F + bf - 1) // bf if bf else 1), "no batch was rebuilt"     # one selection: a build per batch, and the repeats
                assert np.array_equal(bits(rn.table()), bits(rows)) and np.array_equal(rn.sums(), want), bf


def test_next_to_an_rdf_that_repeats_its_batch(emu_lib, oracle):
    overflow_case(emu_lib, oracle)


def next_to_the_other_forms(lib, oracle, device=False):
    """VIAMD's default script plus rmsd, rmsf and clusters statements, with and without the position table in the same IR: every other
    property is bit-identical, the table and the query equal the restatement"""
    atoms, blob, box, F = 3001, 200, 30.0, 4
    coords, topo = TG.blob_system(oracle, n_atoms=atoms, n_blob=blob, box=box, F=F, seed=5)
    el = np.array([str(e).upper() for e in topo.elements])
    wo = np.nonzero((el == "O") & (np.arange(atoms) >= blob))[0].astype(np.int32)
    sites = dict(atoms=wo[:300], groups=np.arange(300, dtype=np.int32), ngroups=300)
    evs = []
    for with_msd in (False, True):
        ir = script.compile_script_native(TG.VIAMD_DEFAULT_SCRIPT + TR.RM_LINE, topo, lib=lib, **OPT_INS)
        ir.add_rmsf("fl", np.arange(blob, dtype=np.int32))
        ir.add_clusters(("ncl", "clsz", "clmax"), sites["atoms"], sites["groups"], CL.R_CUT, ngroups=300)
        if with_msd:
            ir.add_msd(NAME, wo)
        evs.append(TG.evaluate(lib, ir, coords, box, topo.mass, device=device))
    plain, both = evs
    props = plain.ir.property_names()
    assert props == ["d1", "a1", "r", "v", "lin", "plan", "iso", "rm", "fl", "ncl", "clsz", "clmax"]
    assert both.ir.property_names() == props + [NAME]
    for name in props:
        a, b = plain.property_data(name), both.property_data(name)
        assert a.dim == b.dim and a.fingerprint == b.fingerprint, name
        assert np.array_equal(a.values.view(np.int32), b.values.view(np.int32)), name
        if a.c.counts:
            assert np.array_equal(a.counts, b.counts), name
    cells = ((box, box, box), (0.0, 0.0, 0.0), 7)
    rows = R.table(coords, cells, wo)
    pd = both.property_data(NAME)
    assert pd.dim == (F, 3 * wo.size + 9, 0, 0) and pd.unit_str == ("", "Å")
    assert np.array_equal(bits(pd.msd_table), bits(rows))
    assert np.array_equal(both.msd(NAME).sums, R.msd(rows, wo.size, 0, F, F - 1))
    for other in ("rm", "clsz", "r"):
        with pytest.raises(V.VmdError, match="not an msd position table"):
            both.msd(other)


def test_next_to_the_other_forms_on_the_emulator(emu_lib, oracle):
    next_to_the_other_forms(emu_lib, oracle)


# ---- 4. the two-rank merge ------------------------------------------------------------------------------------------------------------------

def _merge_case():
    return MC.lattice_walk(40, 10, seed=13, natoms=50)


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
    coords, atoms = _merge_case()
    F = coords.shape[0]
    beg, end = shard_frames(F, rank, world)
    rn = Run(lib, coords, MC.CUBE8, atoms, device=False, ranges=[(beg, end)])
    own = rn.sums(beg, end)
    reduce_eval(rn.ev)
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), own=own, table=rn.table(), merged=rn.sums(), part=rn.sums(2, 9, 4, 2))
    dist.destroy_process_group()


def test_two_rank_merge(emu_lib, tmp_path):
    """two evals over the halves of the frames, merged through the host collective as the angle table merges: every rank then holds the
    whole table and answers for the whole trajectory - a window across the seam included - with the one-rank sums"""
    import torch.multiprocessing as mp
    port = 57700 + (os.getpid() % 2000)
    mp.spawn(_merge_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    coords, atoms = _merge_case()
    rows = R.table(coords, MC.CUBE8, atoms)
    F = coords.shape[0]
    for r in range(2):
        z = np.load(tmp_path / f"rank{r}.npz")
        beg, end = (0, F // 2) if r == 0 else (F // 2, F)
        assert np.array_equal(z["own"], R.msd(rows, atoms.size, beg, end, end - beg - 1))
        assert np.array_equal(bits(z["table"]), bits(rows))
        assert np.array_equal(z["merged"], R.msd(rows, atoms.size, 0, F, F - 1)) and np.array_equal(z["part"], R.msd(rows, atoms.size, 2, 9, 4, 2))


# ---- 5. host only -----------------------------------------------------------------------------------------------------------------------------

def test_ir_validation_errors(host_lib):
    lib = host_lib
    for sym in ("vmd_ir_add_msd", "vmd_eval_msd", "vmd_eval_msd_atoms", "vmd_hip_msd_gather", "vmd_hip_msd_unwrap", "vmd_hip_msd_lags"):
        assert hasattr(lib, sym), sym
    ir = V.ScriptIR(lib)
    with pytest.raises(V.VmdError, match="atom list is empty"):
        ir.add_msd(NAME, [])
    with pytest.raises(V.VmdError, match="negative atom"):
        ir.add_msd(NAME, [0, 1, -2])
    with pytest.raises(V.VmdError, match="name is empty"):
        ir.add_msd("", [0])
    at = np.array([0, 1], np.int32)
    ip = at.ctypes.data_as(L.c_int32_p)
    assert not lib.vmd_ir_add_msd(None, b"a", ip, 2) and "ir is NULL" in lib.last_error()
    assert not lib.vmd_ir_add_msd(ir.h, None, ip, 2) and "property name" in lib.last_error()
    assert not lib.vmd_ir_add_msd(ir.h, b"a", None, 2) and "empty" in lib.last_error()
    assert not lib.vmd_ir_add_msd(ir.h, b"a", ip, 0) and "empty" in lib.last_error()
    assert ir.property_count() == 0                                                # a refused statement leaves nothing behind
    ir.add_rmsd("g", [0, 1])
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_msd("g", [0, 1])
    ir.add_msd(NAME, [4, 2, 2])                                                    # an atom listed twice is two entries
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_msd(NAME, [0])
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_rmsd(NAME, [0, 1])
    assert ir.property_names() == ["g", NAME] and ir.property_flags(NAME) == L.FLAG_TEMPORAL
    assert list(ir.geometry_atoms(NAME)) == [4, 2, 2] and list(ir.geometry_atoms(NAME, 0)) == [4, 2, 2] and ir.geometry_atoms(NAME, 1).size == 0


def _fnv(h, data):
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_fingerprint_work_and_pins(host_lib):
    assert TR._old_ir(host_lib).fingerprint() == TR.PARENT_FINGERPRINT              # an IR without the form keeps its fingerprint
    # field by field, as vmd_ir_fingerprint hashes a descriptor: the name, the class (TEMPORAL = 2), a, b (none), rmin, rmax, K, m, the form's
    # code 24, aoff = {0, n}; nothing else
    atoms = [5, 1, 9]
    ir = V.ScriptIR(host_lib)
    ir.add_msd(NAME, atoms)
    h = _fnv(0xCBF29CE484222325, NAME.encode())
    h = _fnv(h, struct.pack("<I", 2))
    h = _fnv(h, struct.pack("<3i", *atoms))
    h = _fnv(h, struct.pack("<ff", 0.0, 0.0) + struct.pack("<QQ", 0, 0) + struct.pack("<i", 24) + struct.pack("<2i", 0, 3))
    assert ir.fingerprint() == h

    def fp(name=NAME, atoms=(5, 1, 9)):
        ir = V.ScriptIR(host_lib)
        ir.add_msd(name, list(atoms))
        return ir.fingerprint(), int(host_lib.vmd_ir_work_per_frame(ir.h))
    f0, w0 = fp()
    variants = dict(name=fp(name="x"), atom=fp(atoms=(5, 1, 8)), order=fp(atoms=(1, 5, 9)), fewer=fp(atoms=(5, 1)), more=fp(atoms=(5, 1, 9, 9)))
    assert len({f0} | {v[0] for v in variants.values()}) == 1 + len(variants), variants
    assert w0 == 3 and variants["fewer"][1] == 2
    ir = V.ScriptIR(host_lib)
    ir.add_rmsd(NAME, list(atoms))                                                 # rmsd over the same list is another statement
    assert ir.fingerprint() != f0
    ir = TR._old_ir(host_lib)
    w_old = int(host_lib.vmd_ir_work_per_frame(ir.h))
    ir.add_msd(NAME, [0, 3, 5])
    assert ir.fingerprint() != TR.PARENT_FINGERPRINT and int(host_lib.vmd_ir_work_per_frame(ir.h)) == w_old + 3
    # both pin files are the parent's
    want = {"ir_pin.json": "168e2c1163c8d16b9709d80b54d8ecc66b515fdb0f61260848c3d935eb58878c",
            "script_pin.json": "3e4b6826fd578556e7de3dcf2378ea9c661154b4fa6b0a2d2a336f548ac42635"}
    for fn, digest in want.items():
        with open(os.path.join(ROOT, "tests", "golden", fn), "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == digest, fn


def test_query_refusals_and_exporters(emu_lib):
    lib = emu_lib
    F = 6
    coords, atoms = MC.lattice_walk(4, F, seed=2)
    ir = V.ScriptIR(lib)
    ir.add_rmsd("rm", [0, 1])
    ir.add_msd(NAME, atoms)
    rn = Run(lib, coords, MC.CUBE8, atoms, device=False, ir=ir)
    ok = dict(beg=0, end=F, max_lag=F - 1, stride=1)

    def bad(match, name=NAME, **kw):
        with pytest.raises(V.VmdError, match=match):
            rn.ev.msd(name, **dict(ok, **kw))
    bad("unknown property 'nope'", name="nope")
    bad("'rm' is not an msd position table", name="rm")
    bad("empty or reversed", beg=3, end=3)
    bad("empty or reversed", beg=4, end=2, max_lag=0)
    bad("outside the 6 frames", end=7)
    bad("origin stride must be at least 1", stride=0)
    bad("max_lag 6 needs more than the 6 frames", max_lag=6)
    bad("max_lag 3 needs more than the 3 frames", beg=1, end=4, max_lag=3)
    sums = np.zeros((F, 4), np.uint64)
    sp = sums.ctypes.data_as(L.c_uint64_p)
    assert not lib.vmd_eval_msd(None, NAME.encode(), 0, F, 1, 1, sp, None) and "NULL" in lib.last_error()
    assert not lib.vmd_eval_msd(rn.ev.h, None, 0, F, 1, 1, sp, None) and "NULL" in lib.last_error()
    assert not lib.vmd_eval_msd(rn.ev.h, NAME.encode(), 0, F, 1, 1, None, None) and "NULL" in lib.last_error()
    assert lib.vmd_eval_msd(rn.ev.h, NAME.encode(), 0, F, 1, 1, sp, None) and sums[1, 3] == 5 * 4 and not sums[2:].any()
    assert lib.vmd_eval_msd_atoms(rn.ev.h, NAME.encode()) == 4 and lib.vmd_eval_msd_atoms(rn.ev.h, b"rm") == 0
    # a triclinic cell: the S3t image rounds in fractional space, which the integer unwrap along one axis does not restate - refused
    tilted = Run(lib, coords, ((8.0, 8.0, 8.0), (1.0, 0.0, 0.0), 7), atoms, device=False)
    with pytest.raises(V.VmdError, match="frame 0 has a triclinic cell"):
        tilted.sums()
    # the exporters refuse the table by name
    for fmt in ("csv", "xvg"):
        with pytest.raises(V.VmdError, match="msd position table"):
            rn.ev.export_table("/dev/null", NAME, fmt)
    rn.ev.export_table("/dev/null", "rm", "csv")
    pd = rn.ev.property_data(NAME)
    assert pd.dim == (F, 3 * 4 + 9, 0, 0) and pd.unit_str == ("", "Å")


def test_diffusion_coefficient_recovers_a_line():
    """MSD = 6 D t + c sampled at dt: the slope over the middle lags, over 2 dims, is D exactly (every number below is a dyadic rational)"""
    tau = np.arange(101, dtype=np.float64)
    for D, dt, c, dims in ((0.25, 2.0, 0.0, 3), (0.5, 0.5, 3.0, 3), (0.125, 1.0, -1.0, 2), (2.0, 4.0, 0.5, 1)):
        line = 2 * dims * D * tau * dt + c
        assert diffusion_coefficient(line, dt, dims=dims) == D
        assert diffusion_coefficient(line, dt, lo=0.0, hi=1.0, dims=dims) == D
    # the fit range is [lo, hi] of the largest lag: a kink outside it changes nothing, one inside does
    bent = 6 * 0.25 * tau
    bent[:20] = 0.0
    bent[81:] = 1000.0
    assert diffusion_coefficient(bent, 1.0) == 0.25
    bent[60] += 1.0
    assert diffusion_coefficient(bent, 1.0) != 0.25
    with pytest.raises(ValueError):
        diffusion_coefficient(tau[:3], 1.0, lo=0.4, hi=0.6)
