"""shape_weights() on the MI355X: known answers, the set sizes at the kernels' edges, partly periodic cells, half-cell ties,
the absolute tolerance against both restatements of tests/shape_ref.py at BASELINE sizes, the reduction-order rule under VIAMD's call
patterns, one computation per statement, and VIAMD's default script through the shim with both opt-ins, linked against the product."""
import subprocess

import numpy as np
import pytest

import viamd_amd as V
from viamd_amd import script, synth

import shape_ref as S
import test_geometry as TG
import test_shape as TS

pytestmark = pytest.mark.gpu


def _check_both(got, coords, box, sets, mass, what):
    """against the pinned restatement (the device's own order: expected bit-identical, counted and printed) and the plain one; the bound is
    the same 2^-23 for both"""
    TS.check_tolerance(got, S.values(coords, box, sets, mass), what + " / pinned")
    TS.check_tolerance(got, S.values(coords, box, sets, mass, pinned=False), what + " / plain")


def test_known_answers_on_the_device(gpu_lib):
    TS.known_answers(gpu_lib)


@pytest.mark.parametrize("box,tilt", TS.CELLS)
def test_size_sweep_on_the_device(gpu_lib, box, tilt):
    """the set sizes at which the kernels change path, the unequal populations and the bit identities (alone / in a population / next to
    a large set, resident / host-staged, equal columns) on the hardware's own schedule"""
    TS.size_sweep(gpu_lib, box, tilt, exact=False, device=True)


@pytest.mark.parametrize("box,flags", TS.OPEN_CELLS)
def test_size_sweep_in_partly_periodic_cells_on_the_device(gpu_lib, box, flags):
    TS.size_sweep(gpu_lib, box, flags=flags, exact=False, device=True)


@pytest.mark.parametrize("box,flags", TS.TIE_CELLS)
def test_half_cell_ties_on_the_device(gpu_lib, box, flags):
    TS.half_cell_ties(gpu_lib, box, flags, exact=False, device=True)


def test_water_box_config2(gpu_lib):
    """{l,p,i} = shape_weights(all) and shape_weights(element('O')) on BASELINE config 2's system (100 002 atoms), 1 000 frames resident"""
    atoms, box, F, seed = 100002, 100.0, 1000, 2
    traj = synth.make_device_trajectory(V, seed, atoms, box, F)
    topo = synth.water_box_topology(atoms)
    ir, info = script.compile_script("{l,p,i} = shape_weights(all); {lo,po,io} = shape_weights(element('O'));", topo, shape=True)
    ev = V.ScriptEval(F, ir)
    assert ev.frame_range(V.MolSystem(atoms, mass=topo.mass, unitcell=V.make_unitcell(box)), traj, 0, F)
    sample = sorted(np.random.default_rng(17).choice(F, 12, replace=False).tolist())
    coords = np.stack([traj.download_frame(f)[0] for f in sample])
    assert info["l"]["sets"][0].size == atoms and info["lo"]["sets"][0].size == 33334
    for names in (("l", "p", "i"), ("lo", "po", "io")):
        got = TS.weights(ev, names)
        assert got.shape == (3, F, 1) and np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
        np.testing.assert_allclose(got.astype(np.float64).sum(axis=0), 1.0, atol=3e-7)
        _check_both(got[:, sample], coords, box, info[names[0]]["sets"], topo.mass, f"config 2 {names}")


@pytest.mark.parametrize("tilt", [(0.0, 0.0, 0.0), (12.0, -8.0, 10.0)])
def test_blob_config4_style(gpu_lib, oracle, tilt):
    """shape_weights(resname("ALA")) - one set of all ALA atoms - and shape_weights(all) in resname("ALA") - one set per residue - on the
    config 4-style blob, orthorhombic and tilted cells, every frame"""
    atoms, blob, box, F = 12001, 2000, 50.0, 40
    coords, topo = TG.blob_system(oracle, n_atoms=atoms, n_blob=blob, box=box, F=F, seed=4)
    ir, info = script.compile_script('{lb,pb,ib} = shape_weights(resname("ALA")); {lr,pr,ir} = shape_weights(all) in resname("ALA");', topo,
                                     shape=True)
    cell = V.make_unitcell(box, tilt=tilt)
    traj = V.DeviceTrajectory(F, atoms)
    traj.upload(coords, cell)
    ev = V.ScriptEval(F, ir)
    assert ev.frame_range(V.MolSystem(atoms, mass=topo.mass, unitcell=cell), traj, 0, F)
    bx = (box, box, box) + tuple(tilt)
    assert info["lb"]["sets"][0].size == blob and [s.size for s in info["lr"]["sets"]] == [10] * (blob // 10)
    for names in (("lb", "pb", "ib"), ("lr", "pr", "ir")):
        _check_both(TS.weights(ev, names), coords, bx, info[names[0]]["sets"], topo.mass, f"blob {names} tilt={tilt}")


def test_call_patterns_are_bit_identical_on_the_device(gpu_lib, oracle):
    atoms, blob, box, F = 6001, 1000, 40.0, 60
    coords, topo = TG.blob_system(oracle, n_atoms=atoms, n_blob=blob, box=box, F=F, seed=8)
    ir = script.compile_script(TS.CALL_SCRIPT, topo, shape=True)[0]
    cell = V.make_unitcell(box)
    traj = V.DeviceTrajectory(F, atoms)
    traj.upload(coords, cell)
    sysm = V.MolSystem(atoms, mass=topo.mass, unitcell=cell)

    def run(ranges=None, pooled=None):
        ev = V.ScriptEval(F, ir)
        for beg, end in (ranges or [(0, F)]):
            assert (ev.frame_range_pooled(sysm, traj, beg, end, *pooled) if pooled else ev.frame_range(sysm, traj, beg, end))
        return ev
    TS.call_patterns(gpu_lib, run)


def test_one_computation_per_statement_on_the_device(gpu_lib, oracle):
    coords, topo = TG.blob_system(oracle, n_atoms=6001, n_blob=1000, box=40.0, F=18, seed=8)
    TS.one_computation_per_statement(gpu_lib, coords, topo, 40.0)


def test_shim_default_script_with_both_opt_ins_on_the_gpu(gpu_lib):
    exe = TS.build_shim_shape()
    out = subprocess.run([exe, "24"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("OK frames=24 properties=7 a1=gpu lin=gpu"), out.stdout
