"""rdf() over within() shells on a real MI355X: the scenarios of tests/test_shell_rdf.py through the product library, and
BASELINE config 2's system (100 002 atoms, box 100, 1 000 frames resident, seed 2) - the whole run through the pencil path, sampled
frames one by one against the yardstick on both paths, a run of consecutive frames against the sum of its frames."""
import subprocess

import numpy as np
import pytest

import viamd_amd as V
from viamd_amd import script, synth

import shell_rdf_ref as S
import test_shell_rdf as TS
import test_within as TW

pytestmark = pytest.mark.gpu


def test_known_answers(gpu_lib, oracle):
    TS.known_answers(gpu_lib, oracle)
    TS.known_answers(gpu_lib, oracle, device=True)


def test_radius_exactness(gpu_lib, oracle):
    assert TS.radius_exactness(gpu_lib, oracle, device=True) == 2 * len(TS.RADII)


def test_pencil_brute_and_yardstick_on_the_blob_system(gpu_lib, oracle):
    TS.on_the_blob(gpu_lib, oracle, device=True)


def test_identities(gpu_lib, oracle):
    TS.identities(gpu_lib, oracle, device=True)


def test_switches(gpu_lib, oracle):
    TS.switches(gpu_lib, oracle, device=True)


def test_call_patterns(gpu_lib, oracle):
    TS.call_patterns(gpu_lib, oracle, device=False)
    TS.call_patterns(gpu_lib, oracle, device=True)


def test_a_bucket_overflow_repeats_walk_compaction_and_pass(gpu_lib, oracle):
    TS.overflow_case(gpu_lib, oracle, device=True)


def test_static_rdfs_are_unchanged_by_a_shell_line(gpu_lib, oracle):
    TS.coevaluation(gpu_lib, oracle, device=True)


FULL_SCRIPT = ("g1 = rdf(element('O') and within(3.5, atom(1:300)), element('O'), 10.0);\n"
               "g2 = rdf(element('O') and within(0.5:2.0, element('O')), element('H'), 8.0);")


def sides_of(i):
    sh = lambda s: None if s is None else (s["ref"], s["rmin"], s["rmax"])
    return [(i["ref"], sh(i["ref_shell"])), (i["target"], sh(i["target_shell"]))]


def test_config2_system(gpu_lib, oracle):
    lib = gpu_lib
    n, box, F = 100002, 100.0, 1000
    topo = synth.water_box_topology(n)
    ir, info = script.compile_script(FULL_SCRIPT, topo, lib=lib, shell_rdf=True)
    ir_c = script.compile_script_native(FULL_SCRIPT, topo, lib=lib, shell_rdf=True)
    assert ir.fingerprint() == ir_c.fingerprint()
    cell = V.make_unitcell(box)
    traj = V.DeviceTrajectory(F, n, lib=lib)
    traj.synth(2, box, 0.05)
    sysm = V.MolSystem(n, unitcell=cell)
    # the whole run goes through the pencil path only
    ev = V.ScriptEval(F, ir_c)
    lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
    try:
        assert ev.frame_range(sysm, traj, 0, F) and ev.frame_mask().all()
    finally:
        lib.vmd_profile_enable(False)
    prof = {k: TW.launches(lib, k) for k in TS.PENCIL_KEYS + TS.BRUTE_KEYS}
    assert all(prof[k] >= 2 for k in TS.PENCIL_KEYS) and all(prof[k] == 0 for k in TS.BRUTE_KEYS), prof
    # a dozen sampled frames, one by one, pencil and all pairs, against the yardstick
    frames = [0, 1, 77, 128, 255, 256, 400, 511, 640, 777, 998, 999]
    host = {f: traj.download_frame(f)[0] for f in frames}
    n_checked = 0
    for f in frames:
        one = V.ScriptEval(F, ir_c)
        assert one.frame_range(sysm, traj, f, f + 1)
        with TW.options(lib, force_brute=1):
            brute = V.ScriptEval(F, ir_c)
            assert brute.frame_range(sysm, traj, f, f + 1)
        for name in ("g1", "g2"):
            i = info[name]
            want = S.shell_rdf(oracle, host[f][None], box, sides_of(i), i["rmin"], i["rmax"], method="cells")
            pop = int(want[2][0][0])
            assert 0 < pop < len(i["ref"]) and want[0].sum() > 0, (f, name, pop)
            for e in (one, brute):
                TS.check(lib, oracle, e, name, want, i["rmin"], i["rmax"])
            n_checked += 1
    assert n_checked == 2 * len(frames)
    # a run of 16 consecutive frames equals the sum of its single-frame evaluations
    run = V.ScriptEval(F, ir_c)
    assert run.frame_range(sysm, traj, 300, 316)
    for name in ("g1", "g2"):
        counts, weights, pops = np.zeros(1024, np.uint64), np.zeros(1024, np.float64), set()
        for f in range(300, 316):
            one = V.ScriptEval(F, ir_c)
            assert one.frame_range(sysm, traj, f, f + 1)
            pd = one.property_data(name)
            counts += np.asarray(pd.counts); weights += np.asarray(pd.weights64)
            pops.add(float(np.asarray(pd.weights64).sum()))
        pd = run.property_data(name)
        assert np.array_equal(pd.counts, counts) and counts.sum() > 0 and len(pops) > 1
        np.testing.assert_allclose(pd.weights64, weights, rtol=1e-12, atol=0)


def test_shim_default_script_with_the_shell_line(gpu_lib):
    exe = TS.build_shim_shell_rdf()
    out = subprocess.run([exe, "24"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("OK frames=24 properties=8 gs=gpu fallback_frame_range_calls=0"), out.stdout
    out = subprocess.run([exe, "24", "nobit"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("OK frames=24 properties=8 gs=fallback"), out.stdout + out.stderr[-2000:]
