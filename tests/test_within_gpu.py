"""count(T and within(r, R)) on a real MI355X: the scenarios of tests/test_within.py through the product library, and
BASELINE config 2's system (100 002 atoms, box 100, 1 000 frames resident) against the numpy restatement on sampled frames."""
import os
import subprocess

import numpy as np
import pytest

import viamd_amd as V
from viamd_amd import script, synth

import within_ref as W
import test_within as TW
from test_geometry import rows

pytestmark = pytest.mark.gpu


def test_known_answers(gpu_lib):
    TW.known_answers(gpu_lib)
    TW.known_answers(gpu_lib, device=True)


def test_threshold_exactness(gpu_lib):
    assert TW.threshold_exactness(gpu_lib) == 2 * len(TW.RADII)


def test_both_kernels_on_the_blob_system(gpu_lib, oracle):
    TW.kernels_on_the_blob(gpu_lib, oracle, device=True, F=4)


def test_brute_tile_edges(gpu_lib):
    assert TW.brute_tile_edges(gpu_lib, device=True) == 17


def test_scripts_every_frame(gpu_lib, oracle):
    coords, topo = TW.blob12k(oracle, 4)
    TW.script_parity(gpu_lib, coords, topo, TW.BLOB_SCRIPT, 50.0, device=True)


def test_cross_check_against_rdf(gpu_lib, oracle):
    TW.rdf_cross_check(gpu_lib, oracle, device=True)


def test_call_patterns(gpu_lib, oracle):
    TW.call_patterns(gpu_lib, oracle, device=False)
    TW.call_patterns(gpu_lib, oracle, device=True)


def test_a_bucket_overflow_repeats_the_batch(gpu_lib, oracle):
    TW.overflow_case(gpu_lib, oracle, device=True)


def test_rows_of_temporal_properties_in_an_unusual_order(gpu_lib, oracle):
    TW.row_order_case(gpu_lib, oracle, device=True)


FULL_SCRIPT = ("a = count(element('O') and within(3.5, atom(1:300)));\n"
               "b = count(element('O') and within(0.5:2.0, element('O')));\n"
               "c = count(element('O') and within(1.2:1.8, element('H')));")


def test_config2_system_sampled_frames(gpu_lib):
    """100 002 atoms, box 100, 1 000 frames resident, seed 2: a dozen frames against the restatement, pencil rows == brute rows there"""
    lib = gpu_lib
    n, box, F = 100002, 100.0, 1000
    topo = synth.water_box_topology(n)
    ir, info = script.compile_script(FULL_SCRIPT, topo, lib=lib, within=True)
    cell = V.make_unitcell(box)
    traj = V.DeviceTrajectory(F, n, lib=lib)
    traj.synth(2, box, 0.05)
    sysm = V.MolSystem(n, unitcell=cell)
    lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
    try:
        ev = V.ScriptEval(F, ir)
        assert ev.frame_range(sysm, traj, 0, F) and ev.frame_mask().all()
    finally:
        lib.vmd_profile_enable(False)
    assert TW.launches(lib, "within_pencil") >= 3 and TW.launches(lib, "within_brute") == 0
    frames = [0, 1, 77, 128, 255, 256, 400, 511, 640, 777, 998, 999]
    host = np.stack([traj.download_frame(f)[0] for f in frames])
    with TW.options(lib, force_brute=1):
        brute = V.ScriptEval(F, ir)
        for f in frames:
            assert brute.frame_range(sysm, traj, f, f + 1)
    for name in "abc":
        i = info[name]
        want = W.counts(host, box, i["target"], i["ref"], i["rmin"], i["rmax"], slab=True)
        TW.varied(want, len(i["target"]))
        got = rows(ev, name)[frames, 0]
        print(name, len(i["target"]), len(i["ref"]), want)
        assert np.array_equal(got, want), (name, got, want)
        assert np.array_equal(rows(brute, name)[frames, 0], want), name


def test_shim_default_script_with_the_within_line(gpu_lib):
    exe = TW.build_shim_within()
    out = subprocess.run([exe, "24"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("OK frames=24 properties=8 nw=gpu fallback_frame_range_calls=0"), out.stdout
    out = subprocess.run([exe, "24", "nobit"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("OK frames=24 properties=8 nw=fallback"), out.stdout + out.stderr[-2000:]
