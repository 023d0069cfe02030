"""angle() / dihedral() (DESIGN S6b) on the MI355X: known answers, values at the ends of the range, multi-atom arguments in triclinic
and partly periodic cells, parity with tests/geometry_ref.py at BASELINE sizes, determinism of the call patterns, and VIAMD's default
script through the shim with the angle opt-in, linked against the product."""
import os
import subprocess

import numpy as np
import pytest

import viamd_amd as V
from viamd_amd import script, synth

import geometry_ref as G
import test_geometry as TG

pytestmark = pytest.mark.gpu


def _ulps(a, b):
    """distance in fp32 units in the last place (same-sign finite values)"""
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def _check(got, ref, what):
    u = _ulps(got, ref)
    off = int((u != 0).sum())
    print(f"{what}: {got.size} values, {off} not bit-identical, max {int(u.max())} ulp")
    assert u.max() <= 1, f"{what}: {int(u.max())} ulp from the reference"
    assert off <= max(1, got.size // 1000), f"{what}: {off} values not bit-identical"


def test_known_answers_on_the_device(gpu_lib):
    """exact equalities: `+ 0.0` in k_geom keeps trans at +180 and degenerate input at 0 - a property of the device compile"""
    TG.known_answers(gpu_lib)


def test_values_at_the_ends_of_the_range_on_the_device(gpu_lib):
    TG.range_ends(gpu_lib, exact=False, device=True)


def test_triclinic_cell_on_the_device(gpu_lib):
    TG.triclinic_cell(gpu_lib, exact=False, device=True)


def test_partly_periodic_cell_on_the_device(gpu_lib):
    TG.partly_periodic_cell(gpu_lib, exact=False, device=True)


@pytest.mark.parametrize("geometric", [0, 1])
def test_multi_atom_arguments_and_populations_on_the_device(gpu_lib, oracle, geometric):
    TG.parity(gpu_lib, oracle, geometric, exact=False, device=True)


def test_radians_switch_on_the_device(gpu_lib, oracle):
    TG.radians_switch(gpu_lib, oracle, exact=False, device=True)


def test_water_angle_population_config2(gpu_lib):
    """angle(2,1,3) in resname("HOH") on BASELINE config 2's system (100 002 atoms, 33 334 waters), 1 000 frames resident in HBM"""
    atoms, box, F, seed = 100002, 100.0, 1000, 2
    traj = synth.make_device_trajectory(V, seed, atoms, box, F)
    topo = synth.water_box_topology(atoms)
    ir, info = script.compile_script('a = angle(2,1,3) in resname("HOH");', topo, angles=True)
    ev = V.ScriptEval(F, ir)
    assert ev.frame_range(V.MolSystem(atoms, mass=topo.mass, unitcell=V.make_unitcell(box)), traj, 0, F)
    got = TG.rows(ev, "a")
    assert got.shape == (F, 33334)
    sample = sorted(np.random.default_rng(17).choice(F, 12, replace=False).tolist())
    coords = np.stack([traj.download_frame(f)[0] for f in sample])
    ref = G.values(coords, box, info["a"]["sets"], topo.mass)
    _check(got[sample], ref, "config 2 water angles")
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 180.0


@pytest.mark.parametrize("tilt", [(0.0, 0.0, 0.0), (12.0, -8.0, 10.0)])
def test_blob_dihedral_population(gpu_lib, oracle, tilt):
    """dihedral(1,2,3,4) in resname("ALA") on the config 4-style blob, orthorhombic and tilted cells"""
    atoms, blob, box, F = 12001, 2000, 50.0, 40
    coords, topo = TG.blob_system(oracle, n_atoms=atoms, n_blob=blob, box=box, F=F, seed=4)
    ir, info = script.compile_script('d = dihedral(1,2,3,4) in resname("ALA"); a = angle(2,1,3) in resname("ALA");', topo, angles=True)
    cell = V.make_unitcell(box, tilt=tilt)
    traj = V.DeviceTrajectory(F, atoms)
    traj.upload(coords, cell)
    ev = V.ScriptEval(F, ir)
    assert ev.frame_range(V.MolSystem(atoms, mass=topo.mass, unitcell=cell), traj, 0, F)
    bx = (box, box, box) + tuple(tilt)
    for name in ("d", "a"):
        _check(TG.rows(ev, name), G.values(coords, bx, info[name]["sets"], topo.mass), f"blob {name} tilt={tilt}")


def test_call_patterns_are_bit_identical_on_the_device(gpu_lib, oracle):
    atoms, blob, box, F = 6001, 1000, 40.0, 60
    coords, topo = TG.blob_system(oracle, n_atoms=atoms, n_blob=blob, box=box, F=F, seed=8)
    ir = script.compile_script('d = dihedral(1,2,3,4) in resname("ALA"); a = angle(2,1,3) in resname("ALA"); '
                               'w = angle(2,1,3) in resname("HOH");', topo, angles=True)[0]
    cell = V.make_unitcell(box)
    traj = V.DeviceTrajectory(F, atoms)
    traj.upload(coords, cell)
    sysm = V.MolSystem(atoms, mass=topo.mass, unitcell=cell)

    def run(ranges=None, pooled=None):
        ev = V.ScriptEval(F, ir)
        for beg, end in (ranges or [(0, F)]):
            assert (ev.frame_range_pooled(sysm, traj, beg, end, *pooled) if pooled else ev.frame_range(sysm, traj, beg, end))
        return ev
    one, pool, parts = run(), run(pooled=(16, 1)), run(ranges=[(0, 7), (7, 8), (8, 31), (31, 60)])
    for name in ("d", "a", "w"):
        assert TG.bits_equal(TG.rows(pool, name), TG.rows(one, name)), name
        assert TG.bits_equal(TG.rows(parts, name), TG.rows(one, name)), name


def test_shim_default_script_with_angles_on_the_gpu(gpu_lib):
    exe = TG.build_shim_angles()
    out = subprocess.run([exe, "24"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("OK frames=24 properties=7 a1=gpu"), out.stdout
