"""rmsf on the emulator build and in the host-only entry points: the size edges in three cells against the numpy restatement
(tests/rmsf_ref.py) within its derived bound, the launch choices that must not change a bit (batch size, frame groups, an rmsd property
that lends its sums), planted link shifts, a chain five cells wide, the order of calls, clear_data, the identity with rmsd, frame 0,
degenerate sets, a known answer, a batch repeated for a bucket overflow, the two-rank merge, and the IR cases - every refusal, the
fingerprint field by field, the statement next to the default script and the other forms.  tests/test_rmsf_gpu.py runs the same scenario
functions on the device.  (DESIGN 1.11 sends a new form's IR cases to tests/ir_cases.py; as for 1.12 they stand here.)"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import viamd_amd as V
from viamd_amd import _lib as L
from viamd_amd import script

import cases
import rmsd_ref as RM
import rmsf_cases as RC
import rmsf_ref as R
import test_geometry as TG
import test_rmsd as TR
from test_rama import OPT_INS, Option

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}                       # what -> the worst |difference| / bound seen in this process (printed by every check)


def rmsf_ir(lib, sets, name="f", with_rmsd=False):
    """one rmsf property over `sets` (one index array, or a list of them: a population); with_rmsd: an rmsd property over the same sets
    in front of it, whose sums it then reads"""
    ir = V.ScriptIR(lib)
    single = np.ndim(sets[0]) == 0
    if with_rmsd:
        ir.add_rmsd("g", sets) if single else ir.add_rmsd_population("g", sets)
    if single:
        ir.add_rmsf(name, sets)
    else:
        ir.add_rmsf(name, np.concatenate(sets), np.concatenate([[0], np.cumsum([len(s) for s in sets])]))
    return ir


def record(ev, name="f"):
    return ev.property_data(name).rmsf_accumulators.copy()


def check(got, coords, box, sets, mass, what, flags=7, frames=None, geometric=False):
    """every accumulator within rmsf_ref.bound of the restatement's, the count row exact; vmd_eval_rmsf's formula is checked by the
    callers that have an eval.  Prints the accumulators that differ at all and the worst difference / bound."""
    acc, bnd = R.record(coords, box, sets, mass, geometric=geometric, flags=flags, frames=frames)
    g = R.signed(got)
    assert g.shape == acc.shape, (what, g.shape, acc.shape)
    assert list(g[-1]) == list(acc[-1]), (what, g[-1], acc[-1])
    diff = np.abs((g[:-1] - acc[:-1]).astype(np.float64))
    ratio = np.where(diff == 0.0, 0.0, diff / np.maximum(bnd, 1e-300))
    worst = float(ratio.max()) if ratio.size else 0.0
    WORST[what] = worst
    print(f"{what}: {diff.size} accumulators, {int((diff != 0).sum())} differ from the restatement, worst difference / bound {worst:.3g} "
          f"(largest difference {diff.max() if diff.size else 0:.0f} quanta)")
    assert (diff <= bnd).all(), f"{what}: {worst:.3g} of the bound"
    return acc


def check_reading(ev, name="f"):
    """vmd_eval_rmsf against the same formula applied to the record in numpy: exact up to the last bit of the square root"""
    got = record(ev, name)
    rmsf, mean, frames = ev.rmsf(name)
    want, wmean, wframes = R.read(got)
    assert frames == wframes and np.array_equal(mean, wmean)
    assert np.isfinite(rmsf).all() and (np.abs(rmsf - want) <= np.spacing(want)).all()
    return rmsf


def run(lib, sets, coords, cell, mass=None, device=False, **kw):
    box, tilt, flags = cell
    return TG.evaluate(lib, rmsf_ir(lib, sets, with_rmsd=kw.pop("with_rmsd", False)), coords, box, mass, tilt=tilt, flags=flags, device=device, **kw)


# ---- 1. sizes, cells, launch choices --------------------------------------------------------------------------------------------------------

def size_sweep(lib, ci, device=False):
    """Every size of RC.SIZES as one set and the populations of RC.POPULATIONS in cell ci: the record against the restatement; then the
    same evaluation under every launch choice - batch_frames 1 and 3, every number of frame groups a batch of five frames can have, an
    rmsd property in front that lends its sums - whose records must be the first one's bit for bit."""
    cell = RC.CELLS[ci]
    box, tilt, flags = cell
    bx = tuple(box) + tuple(tilt) if any(tilt) else box
    coords, mass = RC.cloud()
    F = coords.shape[0]
    singles = RC.subsets(10 + ci, RC.SIZES)
    pops = [RC.subsets(20 + 7 * ci + k, sizes) for k, sizes in enumerate(RC.POPULATIONS)]
    for sets in singles + pops:
        what = f"cell {ci}, {len(sets) if np.ndim(sets[0]) == 0 else [len(s) for s in sets]} atoms"
        ev = run(lib, sets, coords, cell, mass, device)
        one = record(ev)
        ntot = one.shape[0] - 1
        assert one[-1, 0] == F and not one[-1, 1:].any(), what
        check(one, coords, bx, sets, mass, what, flags=flags)
        rmsf = check_reading(ev)
        if ntot > 1:
            assert (rmsf > 0.0).any(), what
        if device:
            assert np.array_equal(record(run(lib, sets, coords, cell, mass)), one), f"{what}: resident / host-staged"
        for bf in (1, 3):
            with Option(lib, "batch_frames", bf):
                assert np.array_equal(record(run(lib, sets, coords, cell, mass, device)), one), f"{what}: batch_frames {bf}"
        for groups in range(1, F + 1):
            with Option(lib, "rmsf_frame_groups", groups):
                assert np.array_equal(record(run(lib, sets, coords, cell, mass, device)), one), f"{what}: {groups} frame groups"
        with Option(lib, "rmsf_frame_groups", 2), Option(lib, "batch_frames", 3):
            assert np.array_equal(record(run(lib, sets, coords, cell, mass, device)), one), f"{what}: 2 groups in batches of 3"
        ev2 = run(lib, sets, coords, cell, mass, device, with_rmsd=True)
        assert np.array_equal(record(ev2), one), f"{what}: the sums of an rmsd property"
    assert lib.vmd_set_option(b"rmsf_frame_groups", 0) == 0 and lib.vmd_set_option(b"batch_frames", 0) <= 0


@pytest.mark.parametrize("ci", range(len(RC.CELLS)))
def test_size_edges_on_the_emulator(emu_lib, ci):
    size_sweep(emu_lib, ci)


def test_the_groups_the_host_chooses(host_lib):
    g = host_lib.vmd_hip_rmsf_groups
    assert g(0, 1, 100, 0) == 0 and g(5, 0, 100, 0) == 0
    assert [g(5, 1, 65, w) for w in (1, 2, 3, 4, 5, 6, 99)] == [1, 2, 3, 4, 5, 5, 5]      # asked for: at most one group per frame
    assert g(5, 1, 65, 0) == 5 and g(1000, 1, 100002, 0) == 41 and g(1000, 2000, 10, 0) == 3     # chosen: ~1024 blocks, ~4096 waves
    assert g(1000, 1, 65, 1) == 16 and g(1000, 1, 64, 1) == 1                          # a block's group holds at most 64 frames
    assert g(200, 300000, 65, 0) == 4
    assert host_lib.vmd_hip_rmsf_rot_doubles(7, 3) == 7 * 3 * 15 and host_lib.vmd_hip_rmsf_rot_doubles(0, 3) == 0


# ---- 2. link shifts planted where the scans join; a chain five cells wide -------------------------------------------------------------------

def planted_shifts(lib, device=False):
    """RC.planted: cuts at the first and last lane of a wave, the end of a block's row and both sides of the chunk seam, in a chain whose
    waves otherwise skip their scans.  The record is the restatement's, and the fluctuation is that of the chain without the cuts to
    within the fp32 rounding of coordinates one cell further out."""
    L = 60.0
    cut, whole = RC.planted(L)
    n = cut.shape[2]
    idx = np.arange(n, dtype=np.int32)
    cell = ((L, L, L), (0.0, 0.0, 0.0), 7)
    ev = run(lib, idx, cut, cell, None, device)
    check(record(ev), cut, L, idx, None, "planted shifts")
    a, b = check_reading(ev), check_reading(run(lib, idx, whole, cell, None, device))
    assert not np.array_equal(record(ev), record(run(lib, idx, cut, ((L, L, L), (0.0, 0.0, 0.0), 0), None, device)))     # the cuts are seen
    assert 0.05 < b.min() and b.max() < 0.6 and np.abs(a - b).max() < 1e-4, (b.min(), b.max(), np.abs(a - b).max())
    for groups in (1, 3):
        with Option(lib, "rmsf_frame_groups", groups):
            assert np.array_equal(record(run(lib, idx, cut, cell, None, device)), record(ev)), groups


def test_planted_shifts_on_the_emulator(emu_lib):
    planted_shifts(emu_lib)


def wide_chain(lib, device=False):
    """DESIGN 1.5's case: a chain five cells wide that tumbles.  Frames 1 and 2 are frame 0 turned, moved and jittered by 0.1 A, so every
    atom fluctuates by about that much - against the restatement, and against the whole fp64 chain before wrapping"""
    coords, whole = TR.chain_system()
    idx = np.arange(coords.shape[2], dtype=np.int32)
    ev = run(lib, idx, coords, ((20.0, 20.0, 20.0), (0.0, 0.0, 0.0), 7), None, device)
    check(record(ev), coords, 20.0, idx, None, "chain 5 cells wide under rotation")
    rmsf = check_reading(ev)
    assert 0.01 < np.median(rmsf) < 0.2 and rmsf.max() < 0.5, (np.median(rmsf), rmsf.max())


def test_a_wide_chain_that_tumbles_on_the_emulator(emu_lib):
    wide_chain(emu_lib)


# ---- 3. the order of calls, clear_data ------------------------------------------------------------------------------------------------------

PATTERN_SIZES = [40, 700, RC.CHUNK + 5]


def call_patterns(lib, device=False):
    """frame_range(0, 5) against the ranges (3, 5), (0, 2), (2, 3) - the range with frame 0 is not the first -, pool threads with grain 1
    (read-ahead, frame blocks), a source eval's blocks, and clear_data followed by a second evaluation: all accumulators bit-identical"""
    coords, mass = RC.cloud()
    F = coords.shape[0]
    cell = RC.CELLS[0]
    sets = RC.subsets(31, PATTERN_SIZES)
    ev = run(lib, sets, coords, cell, mass, device)
    one = record(ev)
    assert one[-1, 0] == F and one[:-1].any()
    for kw in (dict(ranges=[(3, 5), (0, 2), (2, 3)]), dict(ranges=[(f, f + 1) for f in range(F)][::-1]), dict(pooled=(16, 1)), dict(pooled=(4, 2))):
        assert np.array_equal(record(run(lib, sets, coords, cell, mass, device, **kw)), one), kw
    vcell = V.make_unitcell(cell[0])
    sysm, traj = V.MolSystem(coords.shape[2], mass=mass, unitcell=vcell), cases.make_traj(lib, coords, vcell, device)
    ev.clear_data()
    assert not record(ev).any() and ev.rmsf("f")[2] == 0 and not ev.rmsf("f")[0].any()
    assert ev.frame_range(sysm, traj, 0, F) and np.array_equal(record(ev), one)
    # a source evaluated in blocks of two frames; a second eval takes frames 2 .. 3 out of its blocks: a partial record
    ir = rmsf_ir(lib, sets)
    src = V.ScriptEval(F, ir)
    src.set_block_frames(2)
    assert src.frame_range(sysm, traj, 0, F) and np.array_equal(record(src), one)
    flt = V.ScriptEval(F, ir)
    flt.set_block_frames(2)
    flt.set_source(src)
    assert flt.frame_range(sysm, traj, 2, 4) and flt.frame_stats()[1] > 0
    part = run(lib, sets, coords, cell, mass, device, ranges=[(2, 4)])
    assert np.array_equal(record(flt), record(part)) and record(part)[-1, 0] == 2
    check(record(part), coords, cell[0], sets, mass, "frames 2 and 3 alone", frames=[2, 3])
    check_reading(part)
    # a frame evaluated twice without clear_data is counted twice, as a ramachandran map counts it
    assert part.frame_range(sysm, traj, 2, 4) and record(part)[-1, 0] == 4 and np.array_equal(record(part)[:-1], 2 * record(flt)[:-1])


def test_call_patterns_on_the_emulator(emu_lib):
    call_patterns(emu_lib)


def many_frames(lib, device=False):
    """48 frames of a three-chunk set in one batch: one group of 48 frames, seven uneven groups, one frame per group (where a step's
    running shifts are read in the iteration after the one that wrote them), and the sums of an rmsd property: one record"""
    coords, mass = RC.cloud(seed=3, frames=48)
    sets = RC.subsets(71, [2 * RC.CHUNK + 1])[0]
    cell = RC.CELLS[0]
    want = None
    for groups in (1, 7, 48, 0):
        with Option(lib, "rmsf_frame_groups", groups):
            got = [record(run(lib, sets, coords, cell, mass, device, with_rmsd=w)) for w in (False, True)]
        want = got[0] if want is None else want
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want), groups
    assert want[-1, 0] == 48
    check(want, coords, cell[0], sets, mass, "48 frames, three chunks")


def test_many_frames_on_the_emulator(emu_lib):
    many_frames(emu_lib)


# ---- 4. the identity with rmsd, frame 0, degenerate sets, a known answer --------------------------------------------------------------------

def identity_with_rmsd(lib, device=False):
    """In one IR with rmsd over the same sets: sum_a w_a |d_a|^2 / W of a one-frame evaluation's column 3 is rmsd^2 of that frame, within
    the sum of the two bounds (rmsd_ref.bound through a^2 - b^2 = (a + b)(a - b); this record's own: the weighted mean of its column-3
    bounds, which hold the quantisation)"""
    coords, mass = RC.cloud()
    cell = RC.CELLS[0]
    sets = RC.subsets(41, [50, 300, RC.CHUNK + 5])
    w_all = mass.astype(np.float64)
    for f in range(1, coords.shape[0]):
        ev = run(lib, sets, coords, cell, mass, device, with_rmsd=True, ranges=[(f, f + 1)])
        got = record(ev)
        assert got[-1, 0] == 1
        _, bnd = R.record(coords, cell[0], sets, mass, frames=[f])
        rmsd = TG.rows(ev, "g")[f].astype(np.float64)
        ref, rb = RM.values(coords, cell[0], sets, mass, frames=[f], pinned=False, with_bound=True)
        k0 = 0
        for c, idx in enumerate(sets):
            w = w_all[idx]
            msd = float(np.sum(w * got[k0:k0 + len(idx), 3].astype(np.float64)) / R.ONE / w.sum())
            own = float(np.sum(w * bnd[k0:k0 + len(idx), 3]) / R.ONE / w.sum())
            other = (rmsd[c] + ref[0, c]) * rb[0, c] + rb[0, c] ** 2
            print(f"frame {f}, set of {len(idx)}: sum w |d|^2 / W {msd:.9g}, rmsd^2 {rmsd[c] ** 2:.9g}, allowed {own + other:.3g}")
            assert abs(msd - rmsd[c] ** 2) <= own + other, (f, c)
            k0 += len(idx)


def test_identity_with_rmsd_on_the_emulator(emu_lib):
    identity_with_rmsd(emu_lib)


def frame_zero_and_degenerate_sets(lib, device=False):
    """Frame 0 alone: an all-zero record with count 1.  A set of one atom and a set whose weights are all zero: zero rows, count F, never
    NaN - next to a live set in the same population, on both routes"""
    coords, mass = RC.cloud()
    F = coords.shape[0]
    cell = RC.CELLS[0]
    for sizes in ([40, 3], [700, 64]):
        sets = RC.subsets(51, sizes)
        got = record(run(lib, sets, coords, cell, mass, device, ranges=[(0, 1)]))
        assert got[-1, 0] == 1 and not got[:-1].any() and not got[-1, 1:].any(), sizes
    m = mass.copy()
    for sizes in ([1, 30, 12], [1, 300, 70]):
        perm = RC.subsets(52, [sum(sizes)])[0]                   # (disjoint sets: the weights of one do not reach another)
        sets = [perm[:1], perm[1:1 + sizes[1]], perm[1 + sizes[1]:]]
        m[:] = mass
        m[sets[2]] = 0.0
        m[sets[1]] = np.maximum(m[sets[1]], 1.0)
        ev = run(lib, sets, coords, cell, m, device)
        got = record(ev)
        assert got[-1, 0] == F and not got[0].any() and not got[1 + sizes[1]:-1].any() and got[1:1 + sizes[1]].any(), sizes
        check(got, coords, cell[0], sets, m, f"degenerate sets {sizes}")
        rmsf = check_reading(ev)
        assert rmsf[0] == 0.0 and not rmsf[1 + sizes[1]:].any() and (rmsf[1:1 + sizes[1]] > 0.0).all()
    # spec_dist_geometric_com: unit weights, so the massless set is live again
    with Option(lib, "spec_dist_geometric_com", 1):
        got = record(run(lib, sets, coords, cell, m, device))
        assert got[1 + sizes[1]:-1].any()
        check(got, coords, cell[0], sets, m, "geometric weights", geometric=True)


def test_frame_zero_and_degenerate_sets_on_the_emulator(emu_lib):
    frame_zero_and_degenerate_sets(emu_lib)


def known_answer(lib, device=False):
    """A rigid copy of the pose under another rotation and translation in every frame.  The pose lies on a 2^-6 grid (exact in fp32); a
    frame's coordinates, all below 32 A in size, are rounded to fp32: at most ulp(32) / 2 = 2^-20 A per axis, eta = sqrt(3) 2^-20 A per
    atom.  After the fit an atom keeps its own rounding, the centroid's (at most eta) and its share of the rotation the least-squares fit
    spends on everybody's rounding (at most 2 eta for a set that is no line: the fit cannot move an atom further than the errors it
    absorbs), and a mean over frames does not exceed the largest term: rmsf <= 4 eta, plus one quantum for the fixed point."""
    pose = TR.CHIRAL + np.array([12.0, 10.0, 9.0])
    rng = np.random.default_rng(5)
    frames = [pose]
    for _ in range(4):
        p = (TR.CHIRAL - TR.CHIRAL.mean(0)) @ RC.rotation(rng).T + rng.uniform(10.0, 20.0, 3)
        assert np.abs(p).max() < 32.0 and p.min() > 0.0
        frames.append(p)
    coords = np.stack([p.T for p in frames]).astype(np.float32)
    idx = np.arange(len(pose), dtype=np.int32)
    ev = run(lib, idx, coords, ((32.0, 32.0, 32.0), (0.0, 0.0, 0.0), 7), None, device)
    check(record(ev), coords, 32.0, idx, None, "rigid copies")
    rmsf, mean, F = ev.rmsf("f")
    limit = 4.0 * math.sqrt(3.0) * 2.0 ** -20 + 2.0 ** -24
    print(f"rigid copies: largest rmsf {rmsf.max():.3g} A, largest mean deviation {np.abs(mean).max():.3g} A, allowed {limit:.3g} A")
    assert F == 5 and rmsf.max() <= limit and np.abs(mean).max() <= limit
    # and one atom moved by 3 A along z in half of the frames: it fluctuates by about 1.5 A, the others far less
    bent = coords.copy()
    bent[[2, 4], 2, -1] += 3.0
    r2 = run(lib, idx, bent, ((32.0, 32.0, 32.0), (0.0, 0.0, 0.0), 0), None, device).rmsf("f")[0]
    assert 1.0 < r2[-1] < 1.6 and r2[:-1].max() < 0.6 * r2[-1], r2


def test_known_answer_on_the_emulator(emu_lib):
    known_answer(emu_lib)


# ---- 5. next to an rdf whose cell build overflows -------------------------------------------------------------------------------------------

def overflow_case(lib, O, device=False):
    """cases.cell_build_overflow_case's construction: the middle frames pile every oxygen into one pencil, a bucket sized from the batch's
    ends overflows and the batch's rdf part is repeated.  The rmsf property of the same IR does not sit behind the overflow flag: its
    frames are counted once, its record is that of an IR without the rdf."""
    n, box, F = 3000, 60.0, 12
    coords = cases.water_box(O, 5, n, box, F)
    o = cases.oxygen(n)
    rng = np.random.default_rng(3)
    for f in (5, 6, 7):
        coords[f][:, o] = rng.uniform(1.0, 11.0, (3, o.size)).astype(np.float32)
    sets = [o[:300], o[300:340]]
    cell = ((box, box, box), (0.0, 0.0, 0.0), 7)
    alone = record(run(lib, sets, coords, cell, None, device))
    with Option(lib, "cells_small", 0), Option(lib, "cells_cap_sample", 2):
        for bf in (0, 4):
            with Option(lib, "batch_frames", bf):
                ir = rmsf_ir(lib, sets)
                ir.add_rdf("goo", o, o, (0.0, 12.0))
                lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
                try:
                    ev = TG.evaluate(lib, ir, coords, box, device=device)
                finally:
                    lib.vmd_profile_enable(False)
                nb = C.c_uint64(0)
                lib.vmd_profile_ms(b"cells_build", C.byref(nb))
                assert nb.value > (F + bf - 1) // bf if bf else nb.value >= 2, "no batch was rebuilt"
                got = record(ev)
                assert got[-1, 0] == F and np.array_equal(got, alone), bf
                lib.vmd_profile_ms(b"rmsf", C.byref(nb))
                assert nb.value == ((F + bf - 1) // bf if bf else 1), "the rmsf launch of a repeated batch ran again"


def test_next_to_an_rdf_that_repeats_its_batch(emu_lib, oracle):
    overflow_case(emu_lib, oracle)


# ---- 6. the two-rank merge ------------------------------------------------------------------------------------------------------------------

def _merge_case():
    coords, mass = RC.cloud()
    return coords, mass, RC.subsets(61, [40, 700, RC.CHUNK + 5])


def _merge_worker(rank, world, port, tmpdir, idle):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import conftest
    from viamd_amd.dist import reduce_eval, shard_frames
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lib = V.VmdLib(conftest.EMU_LIB)
    coords, mass, sets = _merge_case()
    F = coords.shape[0]
    ev = V.ScriptEval(F, rmsf_ir(lib, sets))
    beg, end = (0, F) if idle and rank == 0 else (0, 0) if idle else shard_frames(F, rank, world)
    assert idle or (beg == 0) == (rank == 0)            # only rank 0 holds trajectory frame 0; the other fetches it for the pose
    cell = V.make_unitcell(RC.CELLS[0][0])
    if end > beg:
        assert ev.frame_range(V.MolSystem(coords.shape[2], mass=mass, unitcell=cell), V.HostTrajectory(coords, cell), beg, end)
    own = record(ev)
    reduce_eval(ev)
    rmsf, mean, frames = ev.rmsf("f")
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), own=own, merged=record(ev), rmsf=rmsf, frames=frames, beg=beg, end=end)
    dist.destroy_process_group()


@pytest.mark.parametrize("idle", [False, True])
def test_two_rank_merge(emu_lib, tmp_path, idle):
    """two evals over the halves of the frames (idle: one of them over all frames, the other over none), merged through the host
    collective: every rank's merged record is the one-rank record bit for bit - u64 sums, nothing narrowed - and reads the same"""
    import torch.multiprocessing as mp
    port = 46500 + (os.getpid() % 2000) + (3 if idle else 0)
    mp.spawn(_merge_worker, args=(2, port, str(tmp_path), idle), nprocs=2, join=True)
    coords, mass, sets = _merge_case()
    ev = run(emu_lib, sets, coords, RC.CELLS[0], mass)
    one = record(ev)
    total = np.zeros_like(one)
    for r in range(2):
        z = np.load(tmp_path / f"rank{r}.npz")
        assert z["own"][-1, 0] == int(z["end"]) - int(z["beg"])
        assert (int(z["end"]) > int(z["beg"])) or not z["own"].any()          # a rank without frames contributes zeros
        total = total + z["own"]
        assert np.array_equal(z["merged"], one) and int(z["frames"]) == coords.shape[0]
        assert np.array_equal(z["rmsf"], ev.rmsf("f")[0])
    assert np.array_equal(total, one)


# ---- 7. the IR: every refusal, the fingerprint field by field, the statement next to the others ---------------------------------------------

def test_ir_validation_errors(host_lib):
    lib = host_lib
    for sym in ("vmd_ir_add_rmsf", "vmd_ir_add_rmsf_population", "vmd_eval_rmsf", "vmd_hip_rmsf_fit", "vmd_hip_rmsf_accumulate",
                "vmd_hip_rmsf_groups", "vmd_hip_rmsf_rot_doubles"):
        assert hasattr(lib, sym), sym
    ir = V.ScriptIR(lib)
    with pytest.raises(V.VmdError, match="rmsf context 0 has an empty set"):
        ir.add_rmsf("f", [])
    with pytest.raises(V.VmdError, match="negative"):
        ir.add_rmsf("f", [0, -1])
    with pytest.raises(V.VmdError, match="rmsf context 1 has an empty set"):
        ir.add_rmsf("f", [0], [0, 1, 1])                                           # offsets that do not increase
    with pytest.raises(V.VmdError, match="name is empty"):
        ir.add_rmsf("", [0, 1])
    a = np.array([0, 1], np.int32)
    p = lambda x: x.ctypes.data_as(L.c_int32_p)
    assert not lib.vmd_ir_add_rmsf_population(ir.h, b"x", 2, p(a), p(np.array([1, 2, 3], np.int32)))
    assert "start at 0" in lib.last_error()
    assert not lib.vmd_ir_add_rmsf_population(ir.h, b"x", 0, p(a), p(np.array([0, 1, 2], np.int32)))
    assert "rmsf population is empty" in lib.last_error()
    assert not lib.vmd_ir_add_rmsf_population(ir.h, b"x", 1, p(a), None)
    assert "offsets" in lib.last_error()
    assert not lib.vmd_ir_add_rmsf_population(ir.h, b"x", 1, None, p(np.array([0, 2], np.int32)))
    assert "rmsf set is empty" in lib.last_error()
    assert not lib.vmd_ir_add_rmsf(ir.h, None, p(a), 2)
    assert "name is empty" in lib.last_error()
    assert not lib.vmd_ir_add_rmsf(None, b"x", p(a), 2) and "ir is NULL" in lib.last_error()
    assert not lib.vmd_ir_add_rmsf(ir.h, b"x", p(a), 0x80000000) and "too large" in lib.last_error()
    assert ir.property_count() == 0                                                # a refused statement leaves nothing behind
    ir.add_rmsd("g", [0, 1])
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_rmsf("g", [0, 1])
    ir.add_rmsf("f", [0, 1])
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_rmsd("f", [0, 1])
    assert ir.property_names() == ["g", "f"] and ir.property_flags("f") == L.FLAG_MAP and ir.property_flags("g") == L.FLAG_TEMPORAL
    ir2 = V.ScriptIR(lib)
    ir2.add_rmsf("f", [0, 99])
    if lib.vmd_device_count() > 0:
        with pytest.raises(V.VmdError, match="references atom 99"):
            TG.evaluate(lib, ir2, np.zeros((1, 3, 10), np.float32), 10.0)
        ev = TG.evaluate(lib, ir, np.zeros((2, 3, 10), np.float32), 10.0)
        with pytest.raises(V.VmdError, match="not an rmsf"):
            ev.rmsf("g")
        assert not lib.vmd_eval_rmsf(ev.h, b"nope", None, None, None) and "unknown property" in lib.last_error()
        assert not lib.vmd_eval_rmsf(None, b"f", None, None, None) and "NULL" in lib.last_error()
        assert lib.vmd_eval_rmsf(ev.h, b"f", None, None, None)                     # every output may be left out
        pd = ev.property_data("f")
        assert pd.dim == (3, 4, 0, 0) and pd.unit_str == ("", "Å") and pd.rmsf_accumulators.shape == (3, 4)


def test_fingerprint_work_and_atoms(host_lib):
    assert TR._old_ir(host_lib).fingerprint() == TR.PARENT_FINGERPRINT              # an IR without the form keeps its fingerprint

    def fp(build):
        ir = V.ScriptIR(host_lib)
        build(ir)
        return ir.fingerprint(), int(host_lib.vmd_ir_work_per_frame(ir.h))
    f0, w0 = fp(lambda ir: ir.add_rmsf("g", [0, 1, 2, 3]))
    f_name, _ = fp(lambda ir: ir.add_rmsf("h", [0, 1, 2, 3]))
    f_set, _ = fp(lambda ir: ir.add_rmsf("g", [0, 1, 2, 4]))
    f_order, _ = fp(lambda ir: ir.add_rmsf("g", [0, 2, 1, 3]))                     # the chain runs in the order given
    f_pop, w_pop = fp(lambda ir: ir.add_rmsf("g", [0, 1, 2, 3], [0, 2, 4]))
    f_pop1, _ = fp(lambda ir: ir.add_rmsf("g", [0, 1, 2, 3], [0, 1, 4]))
    f_pop2, w_pop2 = fp(lambda ir: ir.add_rmsf("g", range(8), [0, 3, 4, 8]))
    f_rmsd, w_rmsd = fp(lambda ir: ir.add_rmsd("g", [0, 1, 2, 3]))                 # the form code (13 against 7) and the result class
    f_shape, _ = fp(lambda ir: ir.add_shape_weights(("g", "p", "i"), [0, 1, 2, 3]))
    assert len({f0, f_name, f_set, f_order, f_pop, f_pop1, f_pop2, f_rmsd, f_shape}) == 9
    assert f0 == fp(lambda ir: ir.add_rmsf("g", [0, 1, 2, 3], [0, 4]))[0]          # one context: the single form
    assert (w0, w_pop, w_pop2, w_rmsd) == (8, 8, 16, 4)                            # twice the atoms of every context's set: two passes
    ir = TR._old_ir(host_lib)
    w_old = int(host_lib.vmd_ir_work_per_frame(ir.h))
    ir.add_rmsf("g", range(8), [0, 3, 4, 8])
    assert ir.fingerprint() != TR.PARENT_FINGERPRINT and int(host_lib.vmd_ir_work_per_frame(ir.h)) == w_old + 16
    assert list(ir.geometry_atoms("g")) == [0, 1, 2, 3, 4, 5, 6, 7]
    assert list(ir.geometry_atoms("g", 2)) == [4, 5, 6, 7] and list(ir.geometry_atoms("g", 1)) == [3]
    assert ir.geometry_atoms("g", 3).size == 0


def next_to_the_other_forms(lib, oracle, device=False):
    """VIAMD's default script plus rmsd, ramachandran and secondary_structure statements, with and without an rmsf statement in the same
    IR: every other property is bit-identical, the new one equals the restatement and the record of an IR of its own"""
    atoms, blob, box, F = 6001, 200, 30.0, 8
    coords, topo = TG.blob_system(oracle, n_atoms=atoms, n_blob=blob, box=box, F=F, seed=5)
    names = np.array(["N", "CA", "C", "O", "CB", "H", "HA", "HB1", "CG", "HG"])
    topo.names = np.where(np.arange(atoms) < blob, names[np.arange(atoms) % 10], topo.elements)
    bb = script.backbone_from_topology(topo)
    o = script.backbone_oxygens_from_topology(topo, bb)
    ala = np.arange(blob, dtype=np.int32)
    evs = []
    for with_rmsf in (False, True):
        ir = script.compile_script_native(TG.VIAMD_DEFAULT_SCRIPT + TR.RM_LINE, topo, lib=lib, **OPT_INS)
        ir.add_ramachandran(("bb", "rama"), **bb)
        ir.add_secondary_structure(("ss", "sspop"), bb["n"], bb["ca"], bb["c"], o, bb["range_offsets"], bb["rama_class"])
        if with_rmsf:
            ir.add_rmsf("fl", ala)                                            # the set of `rm`: its sums are shared
            ir.add_rmsf("fr", ala, np.arange(0, blob + 1, 10))                # per residue: one wave per set
        evs.append(TG.evaluate(lib, ir, coords, box, topo.mass, device=device))
    plain, both = evs
    props = plain.ir.property_names()
    assert props == ["d1", "a1", "r", "v", "lin", "plan", "iso", "rm", "bb", "rama", "ss", "sspop"]
    assert both.ir.property_names() == props + ["fl", "fr"]
    for name in props:
        a, b = plain.property_data(name), both.property_data(name)
        assert a.dim == b.dim and a.fingerprint == b.fingerprint, name
        assert np.array_equal(a.values.view(np.int32), b.values.view(np.int32)), name
        if a.c.counts:
            assert np.array_equal(a.counts, b.counts), name
    assert both.ir.property_flags("fl") == L.FLAG_MAP
    sets = [ala[k:k + 10] for k in range(0, blob, 10)]
    check(record(both, "fl"), coords, box, ala, topo.mass, "blob, rmsf(ALA)")
    check(record(both, "fr"), coords, box, sets, topo.mass, "blob, rmsf per residue")
    assert np.array_equal(record(both, "fl"), record(TG.evaluate(lib, rmsf_ir(lib, ala), coords, box, topo.mass, device=device)))
    assert np.array_equal(record(both, "fr"), record(TG.evaluate(lib, rmsf_ir(lib, sets), coords, box, topo.mass, device=device)))
    check_reading(both, "fl")
    # exporters refuse a MAP with a message
    with pytest.raises(V.VmdError, match="rmsf record"):
        both.export_table("/dev/null", "fl", "csv")


def test_next_to_the_other_forms_on_the_emulator(emu_lib, oracle):
    next_to_the_other_forms(emu_lib, oracle)


def test_worst_ratios_are_reported():
    """(runs last in this file: what the checks above measured, in one place)"""
    for what, worst in sorted(WORST.items(), key=lambda kv: -kv[1])[:5]:
        print(f"worst difference / bound {worst:.3g}: {what}")
    assert all(w <= 1.0 for w in WORST.values())
