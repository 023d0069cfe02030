"""sdf() over a within() shell and shell masks on a real MI355X: the scenarios of tests/test_shell_sdf.py through the product
library, and the blob system at the size of BASELINE config 4 (100 001 atoms, a 2 000-atom blob, box 100, seed 4; 1 000 frames resident)
- the whole run through the walk, sampled frames one by one against the yardstick on both paths, a run of consecutive frames against the
sum of its frames, and the masks of three frames through vmd_eval_shell_mask."""
import subprocess

import numpy as np
import pytest

import viamd_amd as V
from viamd_amd import script, synth

import shell_sdf_ref as S
import test_shell_sdf as TS
import test_within as TW
from geometry_ref import Box

pytestmark = pytest.mark.gpu


def test_known_answers(gpu_lib, oracle):
    TS.known_answers(gpu_lib, oracle)
    TS.known_answers(gpu_lib, oracle, device=True)


def test_mask_exactness(gpu_lib, oracle):
    assert TS.mask_exactness(gpu_lib, oracle, device=True) == len(TW.RADII) + 24 + 4


def test_walk_brute_and_yardstick_on_the_blob_system(gpu_lib, oracle):
    TS.on_the_blob(gpu_lib, oracle, device=True)


def test_the_rule_between_walk_and_all_pairs(gpu_lib, oracle):
    TS.mask_rule(gpu_lib, oracle, device=True)


def test_identities(gpu_lib, oracle):
    TS.identities(gpu_lib, oracle, device=True)


def test_call_patterns(gpu_lib, oracle):
    TS.call_patterns(gpu_lib, oracle, device=False)
    TS.call_patterns(gpu_lib, oracle, device=True)


def test_a_bucket_overflow_repeats_the_batch_and_counts_once(gpu_lib, oracle):
    TS.overflow_case(gpu_lib, oracle, device=True)


def test_static_properties_are_unchanged_by_a_shell_sdf_line(gpu_lib, oracle):
    TS.coevaluation(gpu_lib, oracle, device=True)


def test_shell_mask(gpu_lib, oracle):
    TS.shell_mask_product(gpu_lib, oracle, device=False)
    TS.shell_mask_product(gpu_lib, oracle, device=True)


FULL_SCRIPT = ("s = residue(5:11); v = sdf(s, element('O') and water and within(3.5, not water), 10.0);\n"
               "nw = count(element('O') and water and within(3.5, not water));")


def test_config4_system(gpu_lib, oracle):
    lib = gpu_lib
    n, n_blob, box, F = 100001, 2000, 100.0, 1000
    topo = synth.water_box_topology(n, n_blob=n_blob)
    mass = np.asarray(topo.mass, np.float32)
    ir, info = script.compile_script(FULL_SCRIPT, topo, lib=lib, within=True, shell_sdf=True)
    ir_c = script.compile_script_native(FULL_SCRIPT, topo, lib=lib, within=True, shell_sdf=True)
    assert ir.fingerprint() == ir_c.fingerprint()
    i = info["v"]
    sh = i["target_shell"]
    target = (i["target"], (sh["ref"], sh["rmin"], sh["rmax"]))
    cell = V.make_unitcell(box)
    traj = V.DeviceTrajectory(F, n, lib=lib)
    traj.synth(4, box, 0.05, n_blob=n_blob)
    sysm = V.MolSystem(n, mass=mass, unitcell=cell)
    # the whole run goes through the walk only
    ev = V.ScriptEval(F, ir_c)
    lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
    try:
        assert ev.frame_range(sysm, traj, 0, F) and ev.frame_mask().all()
    finally:
        lib.vmd_profile_enable(False)
    prof = {k: TW.launches(lib, k) for k in ("shell_mask", "shell_mask_brute", "sdf_scatter", "cells_build")}
    assert prof["shell_mask"] >= 1 and prof["sdf_scatter"] >= 1 and prof["cells_build"] >= 1 and prof["shell_mask_brute"] == 0, prof
    whole = TS.vol(ev, "v").copy()
    nw = TS.TG.rows(ev, "nw")[:, 0]
    assert whole.sum() > 0 and len(set(nw.tolist())) > 1 and ((nw > 0) & (nw < len(i["target"]))).all()
    # a dozen sampled frames, one by one, walk and all pairs, against the yardstick (the reference pose is frame 0's: host[0] rides along)
    frames = [0, 1, 77, 128, 255, 256, 400, 511, 640, 777, 998, 999]
    host = {f: traj.download_frame(f)[0] for f in frames}
    bx = Box((box, box, box, 0.0, 0.0, 0.0), 7)
    members = {}
    for f in frames:
        pair = np.stack([host[0], host[f]])
        want, pops = S.shell_sdf(oracle, pair, box, i["structures"], mass, target, 10.0, frames=[1])
        static, _ = S.shell_sdf(oracle, pair, box, i["structures"], mass, (i["target"], None), 10.0, frames=[1])
        assert 0 < pops[0] < len(i["target"]) and want.sum() > 0 and (want <= static).all() and not np.array_equal(want, static), (f, pops)
        assert pops[0] == int(nw[f])
        members[f] = int(pops[0])
        one = V.ScriptEval(F, ir_c)
        assert one.frame_range(sysm, traj, f, f + 1)
        with TW.options(lib, force_brute=1):
            brute = V.ScriptEval(F, ir_c)
            assert brute.frame_range(sysm, traj, f, f + 1)
        for e in (one, brute):
            TS.check(e, "v", want, 10.0)
    assert len(set(members.values())) > 1
    # a run of 16 consecutive frames equals the sum of its single-frame evaluations, and the whole run the sum of its halves
    run = V.ScriptEval(F, ir_c)
    assert run.frame_range(sysm, traj, 300, 316)
    total = np.zeros_like(whole)
    for f in range(300, 316):
        one = V.ScriptEval(F, ir_c)
        assert one.frame_range(sysm, traj, f, f + 1)
        total += TS.vol(one, "v")
    assert np.array_equal(TS.vol(run, "v"), total) and total.sum() > 0
    halves = V.ScriptEval(F, ir_c)
    assert halves.frame_range(sysm, traj, 500, F) and halves.frame_range(sysm, traj, 0, 500)
    assert np.array_equal(TS.vol(halves, "v"), whole)
    # the members of three sampled frames by atom
    for f in (0, 400, 999):
        want = S.atom_mask(host[f], bx, target, n)
        got = ev.shell_mask("v", sysm, traj, f)
        assert np.array_equal(got, want) and int(got.sum()) == members[f]
        assert np.array_equal(got, ev.shell_mask("nw", sysm, traj, f))


def test_shim_default_script_with_the_shell_sdf_line(gpu_lib):
    exe = TS.build_shim_shell_sdf()
    out = subprocess.run([exe, "24"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("OK frames=24 properties=8 gs=gpu fallback_frame_range_calls=0"), out.stdout
    out = subprocess.run([exe, "24", "nobit"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("OK frames=24 properties=8 gs=fallback"), out.stdout + out.stderr[-2000:]
