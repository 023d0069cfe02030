"""Residue contact maps and the native-contact fraction on the MI355X: the scenario functions of tests/test_contacts.py
through the product library, resident trajectories (the size sweep also checks resident against host-staged).  The rule is the emulator's:
the counts, every accumulator, the Q floats and the pair lists EXACTLY equal to the numpy restatement, every launch choice bit-identical;
each check prints how many candidate entry pairs lie within 4 ulp of r_cut.  What stays with the CPU suite is the host-only part (the IR
cases, the topology helper) and the two-rank merge through gloo."""
import pytest

import contact_cases as CC
import test_contacts as T

pytestmark = pytest.mark.gpu


def test_known_answers_on_the_device(gpu_lib):
    T.known_answers(gpu_lib, device=True)


@pytest.mark.parametrize("ci", range(len(CC.CELLS)))
def test_size_edges_on_the_device(gpu_lib, ci):
    T.size_sweep(gpu_lib, ci, device=True)


def test_largest_index_on_the_device(gpu_lib):
    T.largest_index(gpu_lib, device=True)


def test_lds_rows_on_the_device(gpu_lib):
    T.lds_rows(gpu_lib, device=True)


def test_duplicates_on_the_device(gpu_lib):
    T.duplicates(gpu_lib, device=True)


def test_thresholds_on_the_device(gpu_lib):
    T.thresholds(gpu_lib, device=True)
    met = {k: v for k, v in T.NEAR.items() if k.startswith("thresholds")}
    assert met and all(v >= 8 for v in met.values())


def test_tight_boxes_on_the_device(gpu_lib):
    T.tight_boxes(gpu_lib, device=True)


def test_identity_on_the_device(gpu_lib):
    T.identity(gpu_lib, device=True)


def test_native_fraction_on_the_device(gpu_lib):
    T.native_q(gpu_lib, device=True)


def test_call_patterns_on_the_device(gpu_lib):
    T.call_patterns(gpu_lib, device=True)
    T.call_patterns(gpu_lib)


def test_reader_under_every_name_on_the_device(gpu_lib):
    T.reader_names(gpu_lib, device=True)


def test_next_to_an_rdf_that_repeats_its_batch_on_the_device(gpu_lib, oracle):
    T.overflow_case(gpu_lib, oracle, device=True)


def test_next_to_the_other_forms_on_the_device(gpu_lib, oracle):
    T.next_to_the_other_forms(gpu_lib, oracle, device=True)
