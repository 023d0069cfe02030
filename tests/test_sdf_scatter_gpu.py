"""The cases of tests/sdf_scatter_cases.py on the MI355X, from a trajectory resident in HBM: what the emulator cannot show - __syncthreads,
the LDS atomics and the ballots of the round loops on real waves, the real grids."""
import pytest

import sdf_scatter_cases as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ntgt", D.TARGET_COUNTS)
def test_target_count_against_the_tiles_on_the_device(gpu_lib, oracle, ntgt):
    D.target_count(gpu_lib, oracle, ntgt, device=True)


@pytest.mark.parametrize("ntgt", D.ILP_COUNTS)
def test_target_count_against_the_tiles_of_8_and_16_per_thread_on_the_device(gpu_lib, oracle, ntgt):
    D.ilp_target_count(gpu_lib, oracle, ntgt, device=True)


@pytest.mark.parametrize("n_near", D.BLOCK_NEAR)
def test_block_rounds_on_the_device(gpu_lib, oracle, n_near):
    D.block_rounds(gpu_lib, oracle, n_near, device=True)


@pytest.mark.parametrize("n_near", D.WAVE_NEAR)
def test_wave_rounds_on_the_device(gpu_lib, oracle, n_near):
    D.wave_rounds(gpu_lib, oracle, n_near, device=True)


@pytest.mark.parametrize("ntgt,frames", D.STREAM_WALKS)
def test_stream_walk_on_the_device(gpu_lib, oracle, ntgt, frames):
    D.stream_walk(gpu_lib, oracle, ntgt, frames, device=True)


def test_rows_shapes_on_the_device(gpu_lib, oracle):
    D.rows_shapes(gpu_lib, oracle, device=True)


def test_dense_shapes_on_the_device(gpu_lib, oracle):
    D.dense_shapes(gpu_lib, oracle, device=True)


def test_seven_structures_on_the_device(gpu_lib, oracle):
    D.seven_structures(gpu_lib, oracle, device=True)


def test_targets_include_the_structures_own_atoms_on_the_device(gpu_lib, oracle):
    D.own_atoms(gpu_lib, oracle, device=True)
