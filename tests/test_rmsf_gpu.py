"""rmsf on the MI355X: the scenario functions of tests/test_rmsf.py through the product library, resident trajectories (the
size sweep also checks resident against host-staged).  The rule is the emulator's: every accumulator within rmsf_ref.bound of the numpy
restatement, every launch choice bit-identical.  Each check prints how many accumulators differ from the restatement at all and the
worst difference / bound.  No case of tests/test_rmsf.py's scenarios is left out on the device; what stays with the CPU suite is the
host-only part (the IR cases, the host's choice of groups) and the two-rank merge through gloo."""
import pytest

import rmsf_cases as RC
import test_rmsf as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ci", range(len(RC.CELLS)))
def test_size_edges_on_the_device(gpu_lib, ci):
    T.size_sweep(gpu_lib, ci, device=True)


def test_planted_shifts_on_the_device(gpu_lib):
    T.planted_shifts(gpu_lib, device=True)


def test_a_wide_chain_that_tumbles_on_the_device(gpu_lib):
    T.wide_chain(gpu_lib, device=True)


def test_call_patterns_on_the_device(gpu_lib):
    T.call_patterns(gpu_lib, device=True)
    T.call_patterns(gpu_lib)


def test_many_frames_on_the_device(gpu_lib):
    T.many_frames(gpu_lib, device=True)


def test_identity_with_rmsd_on_the_device(gpu_lib):
    T.identity_with_rmsd(gpu_lib, device=True)


def test_frame_zero_and_degenerate_sets_on_the_device(gpu_lib):
    T.frame_zero_and_degenerate_sets(gpu_lib, device=True)


def test_known_answer_on_the_device(gpu_lib):
    T.known_answer(gpu_lib, device=True)


def test_next_to_an_rdf_that_repeats_its_batch_on_the_device(gpu_lib, oracle):
    T.overflow_case(gpu_lib, oracle, device=True)


def test_next_to_the_other_forms_on_the_device(gpu_lib, oracle):
    T.next_to_the_other_forms(gpu_lib, oracle, device=True)


def test_worst_ratios_on_the_device():
    T.test_worst_ratios_are_reported()
