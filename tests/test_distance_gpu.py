"""The cases of tests/distance_cases.py on the MI355X, from a trajectory resident in HBM: what the emulator cannot show - __syncthreads and
LDS in the reduction of k_distance_minmax, the real grid decomposition of k_distance_com and k_distance_pair."""
import pytest

import distance_cases as D

pytestmark = pytest.mark.gpu


def test_minmax_planted_extremum_on_the_device(gpu_lib, oracle):
    D.minmax_planted_extremum(gpu_lib, oracle, device=True)


def test_minmax_pair_count_edges_on_the_device(gpu_lib, oracle):
    D.minmax_pair_count_edges(gpu_lib, oracle, device=True)


def test_ragged_populations_on_the_device(gpu_lib, oracle):
    D.ragged_populations(gpu_lib, oracle, device=True)


def test_com_slots_on_the_device(gpu_lib, oracle):
    D.com_slots(gpu_lib, oracle, device=True)


def test_com_large_set_on_the_device(gpu_lib, oracle):
    D.com_large_set(gpu_lib, oracle, device=True)


def test_pair_populations_on_the_device(gpu_lib, oracle):
    D.pair_populations(gpu_lib, oracle, device=True)


def test_batching_on_the_device(gpu_lib, oracle):
    D.batching(gpu_lib, oracle, device=True)


def test_triclinic_on_the_device(gpu_lib, oracle):
    D.triclinic(gpu_lib, oracle, device=True)


def test_script_level_on_the_device(gpu_lib, oracle):
    D.script_level(gpu_lib, oracle, device=True)
