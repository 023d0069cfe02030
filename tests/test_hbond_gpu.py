"""Hydrogen bonds on the MI355X: the scenario functions of tests/test_hbond.py through the product library, resident
trajectories (the size sweep also checks resident against host-staged).  The rule is the emulator's: the counts, every accumulator and the
pair lists EXACTLY equal to the numpy restatement, every launch choice bit-identical; each check prints how many candidate pairs lie within
4 ulp of either threshold.  What stays with the CPU suite is the host-only part (the IR cases, the topology helper) and the two-rank merge
through gloo."""
import pytest

import hbond_cases as HC
import test_hbond as T

pytestmark = pytest.mark.gpu


def test_known_answer_on_the_device(gpu_lib):
    T.known_answer(gpu_lib, device=True)


@pytest.mark.parametrize("ci", range(len(HC.CELLS)))
def test_size_edges_on_the_device(gpu_lib, ci):
    T.size_sweep(gpu_lib, ci, device=True)


def test_tight_boxes_on_the_device(gpu_lib):
    T.tight_boxes(gpu_lib, device=True)


def test_thresholds_on_the_device(gpu_lib):
    T.thresholds(gpu_lib, device=True)


def test_identity_on_the_device(gpu_lib):
    T.identity(gpu_lib, device=True)


def test_sorted_atoms_leaves_no_slot_unclaimed_on_the_device(gpu_lib, oracle):
    T.sorted_atoms_identity(gpu_lib, oracle, gpu=True)


def test_call_patterns_on_the_device(gpu_lib):
    T.call_patterns(gpu_lib, device=True)
    T.call_patterns(gpu_lib)


def test_next_to_an_rdf_that_repeats_its_batch_on_the_device(gpu_lib, oracle):
    T.overflow_case(gpu_lib, oracle, device=True)


def test_next_to_the_other_forms_on_the_device(gpu_lib, oracle):
    T.next_to_the_other_forms(gpu_lib, oracle, device=True)


def test_thresholds_were_exercised_on_the_device():
    T.test_thresholds_were_exercised()
