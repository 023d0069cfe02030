"""Connected clusters of groups per frame on the MI355X: the scenario functions of tests/test_clusters.py through the
product library, resident trajectories (the size sweep also checks resident against host-staged).  The rule is the emulator's: the counts,
the largest sizes, every accumulator and every label EXACTLY equal to the numpy restatement, every launch choice bit-identical; each check
prints how many entry pairs lie within 4 ulp of r_cut.  Here - contention first - is where the CONCURRENCY of the lock-free union is
checked: the emulator runs one lane at a time.  What stays with the CPU suite is the host-only part (the IR cases) and the two-rank merge
through gloo; what runs here alone is the 5 000-group case."""
import pytest

import cluster_cases as CL
import test_clusters as T

pytestmark = pytest.mark.gpu


def test_contention_on_the_device(gpu_lib):
    T.contention(gpu_lib, device=True)


def test_known_answers_on_the_device(gpu_lib):
    T.known_answers(gpu_lib, device=True)


def test_lines_on_the_device(gpu_lib):
    T.lines(gpu_lib, device=True)


def test_thresholds_on_the_device(gpu_lib):
    T.thresholds(gpu_lib, device=True)
    met = {k: v for k, v in T.NEAR.items() if k.startswith("thresholds")}
    assert met and all(v >= 8 for v in met.values())


def test_tight_boxes_on_the_device(gpu_lib):
    T.tight_boxes(gpu_lib, device=True)


@pytest.mark.parametrize("ci", range(len(CL.CELLS)))
def test_size_edges_on_the_device(gpu_lib, ci):
    T.size_sweep(gpu_lib, ci, device=True)


def test_five_thousand_groups_on_the_device(gpu_lib):
    T.many_groups(gpu_lib, device=True)


def test_identity_on_the_device(gpu_lib):
    T.identity(gpu_lib, device=True)


def test_call_patterns_on_the_device(gpu_lib):
    T.call_patterns(gpu_lib, device=True)
    T.call_patterns(gpu_lib)


def test_two_statements_over_one_list_on_the_device(gpu_lib):
    T.two_radii(gpu_lib, device=True)


def test_readers_under_every_name_on_the_device(gpu_lib):
    T.reader_names(gpu_lib, device=True)


def test_next_to_an_rdf_that_repeats_its_batch_on_the_device(gpu_lib, oracle):
    T.overflow_case(gpu_lib, oracle, device=True)


def test_next_to_the_other_forms_on_the_device(gpu_lib, oracle):
    T.next_to_the_other_forms(gpu_lib, oracle, device=True)
