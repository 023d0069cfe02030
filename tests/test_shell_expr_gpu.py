"""and / or / not over within() shells on a real MI355X: the scenarios of tests/test_shell_expr.py through the product
library, host and device trajectories, and VIAMD's default script plus the two expression lines through the shim."""
import subprocess

import pytest

import test_shell_expr as TE

pytestmark = pytest.mark.gpu


def test_known_answers(gpu_lib):
    TE.known_answers(gpu_lib)
    TE.known_answers(gpu_lib, device=True)


@pytest.mark.parametrize("cell", ["cubic", "tilted", "slab"])
def test_the_blob_expressions(gpu_lib, oracle, cell):
    TE.on_the_blob(gpu_lib, oracle, device=True, cells=(cell,))


def test_both_twins_on_the_blob_system(gpu_lib, oracle):
    TE.twins_on_the_blob(gpu_lib, oracle, device=True)


def test_kernel_edges(gpu_lib, oracle):
    TE.kernel_edges(gpu_lib, oracle, device=True)


def test_identities(gpu_lib, oracle):
    TE.identities(gpu_lib, oracle, device=True)


def test_sdf_against_the_yardstick(gpu_lib, oracle):
    TE.sdf_against_the_yardstick(gpu_lib, oracle, device=True)


def test_a_bucket_overflow_repeats_the_batch_and_counts_once(gpu_lib, oracle):
    TE.overflow_case(gpu_lib, oracle, device=True)


def test_call_patterns(gpu_lib, oracle):
    TE.call_patterns(gpu_lib, oracle, device=False)
    TE.call_patterns(gpu_lib, oracle, device=True)


def test_static_properties_are_unchanged_by_expression_lines(gpu_lib, oracle):
    TE.coevaluation(gpu_lib, oracle, device=True)


def test_shim_default_script_with_the_expression_lines(gpu_lib):
    exe = TE.build_shim_shell_expr()
    out = subprocess.run([exe, "24"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("OK frames=24 properties=9 expr=gpu fallback_frame_range_calls=0"), out.stdout
    out = subprocess.run([exe, "24", "nobit"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.startswith("OK frames=24 properties=9 expr=fallback") and "fallback_frame_range_calls=0" not in out.stdout, out.stdout
