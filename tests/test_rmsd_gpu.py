"""rmsd() on the MI355X: known answers and the chain that tumbles, the set sizes at the kernels' edges, partly periodic
cells, half-cell ties, the derived tolerance against both restatements of tests/rmsd_ref.py at BASELINE sizes, the reduction-order rule
under VIAMD's call patterns, the pose's lifetime, and VIAMD's default script plus an rmsd line through the shim with the three opt-ins,
linked against the product."""
import subprocess

import numpy as np
import pytest

import viamd_amd as V
from viamd_amd import script, synth

import test_geometry as TG
import test_rmsd as TR

pytestmark = pytest.mark.gpu


def test_known_answers_on_the_device(gpu_lib):
    TR.known_answers(gpu_lib)


def test_a_wide_chain_that_tumbles_on_the_device(gpu_lib):
    TR.wide_chain(gpu_lib)


@pytest.mark.parametrize("box,tilt", TR.CELLS)
def test_size_sweep_on_the_device(gpu_lib, box, tilt):
    """the set sizes at which the kernels change path (the chunk seams with their carried-in shifts among them), the unequal populations
    and the bit identities (alone / in a population / next to a large set, resident / host-staged, equal columns) on the hardware's
    own schedule"""
    TR.size_sweep(gpu_lib, box, tilt, exact=False, device=True)


@pytest.mark.parametrize("box,flags", TR.OPEN_CELLS)
def test_size_sweep_in_partly_periodic_cells_on_the_device(gpu_lib, box, flags):
    TR.size_sweep(gpu_lib, box, flags=flags, exact=False, device=True)


@pytest.mark.parametrize("box,flags", TR.TS.TIE_CELLS)
def test_half_cell_ties_on_the_device(gpu_lib, box, flags):
    TR.half_cell_ties(gpu_lib, box, flags, exact=False, device=True)


def test_water_box_config2(gpu_lib):
    """rmsd(all) and rmsd(element('O')) on BASELINE config 2's system (100 002 atoms), 1 000 frames resident.  The frames are drawn
    independently, so this is a test of loads and arithmetic (the chain runs through unrelated molecules, the accumulated shifts wander
    over thousands of cells, the value is ~1e4 A), not of physics: a dozen sampled frames against both restatements, bound as derived;
    bit-identity with the pinned one is counted and printed, not required."""
    atoms, box, F, seed = 100002, 100.0, 1000, 2
    traj = synth.make_device_trajectory(V, seed, atoms, box, F)
    topo = synth.water_box_topology(atoms)
    ir, info = script.compile_script("g = rmsd(all); go = rmsd(element('O'));", topo, rmsd=True)
    ev = V.ScriptEval(F, ir)
    assert ev.frame_range(V.MolSystem(atoms, mass=topo.mass, unitcell=V.make_unitcell(box)), traj, 0, F)
    sample = [0] + sorted((1 + np.random.default_rng(17).choice(F - 1, 12, replace=False)).tolist())
    coords = np.stack([traj.download_frame(f)[0] for f in sample])                # coords[0] is trajectory frame 0: the pose
    assert info["g"]["sets"][0].size == atoms and info["go"]["sets"][0].size == 33334
    for name in ("g", "go"):
        got = TR.rows(ev, name)
        assert got.shape == (F, 1) and np.isfinite(got).all() and got.view(np.int32)[0, 0] == 0 and got[1:].min() > 0.0
        TR.check_tolerance(got[sample], coords, box, info[name]["sets"], topo.mass, f"config 2 {name}")


@pytest.mark.parametrize("tilt", [(0.0, 0.0, 0.0), (12.0, -8.0, 10.0)])
def test_blob_config4_style(gpu_lib, oracle, tilt):
    """rmsd(resname("ALA")) - one set of all ALA atoms - and rmsd(all) in resname("ALA") - one set per residue - on the config 4-style
    blob, orthorhombic and tilted cells, every frame"""
    atoms, blob, box, F = 12001, 2000, 50.0, 40
    coords, topo = TG.blob_system(oracle, n_atoms=atoms, n_blob=blob, box=box, F=F, seed=4)
    ir, info = script.compile_script('gb = rmsd(resname("ALA")); gr = rmsd(all) in resname("ALA");', topo, rmsd=True)
    cell = V.make_unitcell(box, tilt=tilt)
    traj = V.DeviceTrajectory(F, atoms)
    traj.upload(coords, cell)
    ev = V.ScriptEval(F, ir)
    assert ev.frame_range(V.MolSystem(atoms, mass=topo.mass, unitcell=cell), traj, 0, F)
    bx = (box, box, box) + tuple(tilt)
    assert info["gb"]["sets"][0].size == blob and [s.size for s in info["gr"]["sets"]] == [10] * (blob // 10)
    for name in ("gb", "gr"):
        got = TR.rows(ev, name)
        assert not got.view(np.int32)[0].any() and got[1:].min() > 0.0
        TR.check_tolerance(got, coords, bx, info[name]["sets"], topo.mass, f"blob {name} tilt={tilt}")


def test_script_populations_on_the_device(gpu_lib, oracle):
    coords, topo = TG.blob_system(oracle)
    TR.script_populations(gpu_lib, coords, topo, (30.0, 30.0, 30.0), what="device blob")
    TR.script_populations(gpu_lib, coords, topo, (30.0, 30.0, 30.0), tilt=(6.0, -3.0, 9.0), geometric=1, what="device blob")


def test_call_patterns_are_bit_identical_on_the_device(gpu_lib, oracle):
    atoms, blob, box, F = 6001, 1000, 40.0, 60
    coords, topo = TG.blob_system(oracle, n_atoms=atoms, n_blob=blob, box=box, F=F, seed=8)
    ir = script.compile_script(TR.CALL_SCRIPT, topo, rmsd=True)[0]
    cell = V.make_unitcell(box)
    traj = V.DeviceTrajectory(F, atoms)
    traj.upload(coords, cell)
    sysm = V.MolSystem(atoms, mass=topo.mass, unitcell=cell)

    def run(ranges=None, pooled=None):
        ev = V.ScriptEval(F, ir)
        for beg, end in (ranges or [(0, F)]):
            assert (ev.frame_range_pooled(sysm, traj, beg, end, *pooled) if pooled else ev.frame_range(sysm, traj, beg, end))
        return ev
    one = TR.call_patterns(gpu_lib, run)
    # the same rows from a host trajectory (frames staged batch by batch) and from the resident one
    host = TG.evaluate(gpu_lib, ir, coords, box, topo.mass)
    for name in TR.CALL_NAMES:
        assert TR.bits_equal(TR.rows(host, name), TR.rows(one, name)), name


def test_pose_lifetime_on_the_device(gpu_lib, oracle):
    coords_a, topo = TG.blob_system(oracle, F=6)
    coords_b, _ = TG.blob_system(oracle, F=6, seed=9)
    TR.pose_lifetime(gpu_lib, coords_a, coords_b, topo)


def test_shim_default_script_with_the_rmsd_line_on_the_gpu(gpu_lib):
    exe = TR.build_shim_rmsd()
    out = subprocess.run([exe, "24"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("OK frames=24 properties=8 rm=gpu fallback_frame_range_calls=0"), out.stdout
    out = subprocess.run([exe, "24", "nobit"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("OK frames=24 properties=8 rm=fallback"), out.stdout
