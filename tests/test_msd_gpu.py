"""Mean-squared displacement over lag times on the MI355X: the scenario functions of tests/test_msd.py through the product
library, over host trajectories (vmd_hosttraj_*) and, for the call patterns and the size edges, resident ones.  The rule is the emulator's:
the table's rows equal the frame's floats bit for bit and every u64 of the query equals the NumPy restatement EXACTLY.  Here - many blocks
first - is where the CONCURRENCY is checked: thousands of lanes add to the same lag rows with 64-bit atomics, which the emulator, one lane
at a time, cannot show.  What stays with the CPU suite is the host-only part and the two-rank merge through gloo."""
import pytest

import test_msd as T

pytestmark = pytest.mark.gpu


def test_many_blocks_on_the_device(gpu_lib):
    T.many_blocks(gpu_lib)


def test_known_answers_on_the_device(gpu_lib):
    T.known_answers(gpu_lib)
    T.known_answers(gpu_lib, device=True)


def test_size_edges_on_the_device(gpu_lib):
    T.size_sweep(gpu_lib)


def test_size_edges_with_a_cell_per_frame_on_the_device(gpu_lib):
    T.size_sweep(gpu_lib, device=True, breathing=True)


def test_a_frame_with_a_dead_edge_on_the_device(gpu_lib):
    T.dead_edge(gpu_lib)
    T.dead_edge(gpu_lib, device=True)


def test_lag_chunks_on_the_device(gpu_lib):
    T.lag_chunks(gpu_lib)


def test_non_lattice_coordinates_on_the_device(gpu_lib):
    T.liquid(gpu_lib)
    T.liquid(gpu_lib, device=True)


def test_call_patterns_on_the_device(gpu_lib):
    T.call_patterns(gpu_lib)
    T.call_patterns(gpu_lib, device=True)


def test_next_to_an_rdf_that_repeats_its_batch_on_the_device(gpu_lib, oracle):
    T.overflow_case(gpu_lib, oracle)


def test_next_to_the_other_forms_on_the_device(gpu_lib, oracle):
    T.next_to_the_other_forms(gpu_lib, oracle, device=True)
