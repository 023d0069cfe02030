"""Solvent-accessible surface area on the MI355X: the scenario functions of tests/test_sasa.py through the product library,
resident trajectories (the size sweep also checks resident against host-staged).  The rule is the emulator's: the point counts, every
accumulator, the u64 totals and the temporal floats EXACTLY equal to the numpy restatement, every launch choice bit-identical; each check
prints how many candidate pairs lie within 4 ulp of s * s and how many point tests within 4 ulp of t_ij.  What stays with the CPU suite is
the host-only part (the IR cases, the point table, the radii helper) and the two-rank merge through gloo."""
import pytest

import sasa_cases as SC
import test_sasa as T

pytestmark = pytest.mark.gpu


def test_known_answers_on_the_device(gpu_lib):
    T.known_answers(gpu_lib, device=True)
    T.two_spheres(gpu_lib, device=True)
    T.interface_area(gpu_lib, device=True)


def test_hand_placed_pairs_on_the_device(gpu_lib):
    T.hand_placed_pairs(gpu_lib, device=True)


@pytest.mark.parametrize("ci", range(len(SC.CELLS)))
def test_size_edges_on_the_device(gpu_lib, ci):
    T.size_sweep(gpu_lib, ci, device=True)


def test_npoints_edges_on_the_device(gpu_lib):
    T.npoints_edges(gpu_lib, device=True)


def test_tight_boxes_on_the_device(gpu_lib):
    T.tight_boxes(gpu_lib, device=True)


def test_thresholds_on_the_device(gpu_lib):
    T.thresholds(gpu_lib, device=True)
    T.mixed_radii(gpu_lib, device=True)


def test_identity_on_the_device(gpu_lib):
    T.identity(gpu_lib, device=True)


def test_call_patterns_on_the_device(gpu_lib):
    T.call_patterns(gpu_lib, device=True)
    T.call_patterns(gpu_lib)


def test_next_to_an_rdf_that_repeats_its_batch_on_the_device(gpu_lib, oracle):
    T.overflow_case(gpu_lib, oracle, device=True)


def test_next_to_the_other_forms_on_the_device(gpu_lib, oracle):
    T.next_to_the_other_forms(gpu_lib, oracle, device=True)

