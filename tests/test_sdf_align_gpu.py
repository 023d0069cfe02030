"""The cases of tests/sdf_align_cases.py on the MI355X: what the emulator cannot show - the device's fp64 division, square root and
contraction in the Jacobi sweeps, the real grid decomposition of k_sdf_align and k_sdf_group over more than one block, the scratch
offsets of the tree walk in device memory.  Every case prints its worst deviation from the fp64 reference in units of u."""
import pytest

import sdf_align_cases as A

pytestmark = pytest.mark.gpu


def test_thread_slots_on_the_device(gpu_lib):
    A.thread_slots(gpu_lib, device=True)


def test_structure_sizes_on_the_device(gpu_lib):
    A.structure_sizes(gpu_lib, device=True)


def test_masses_on_the_device(gpu_lib):
    A.masses(gpu_lib, device=True)


def test_unwrap_chain_on_the_device(gpu_lib):
    A.unwrap_chain(gpu_lib, device=True)


def test_unwrap_tree_on_the_device(gpu_lib):
    A.unwrap_tree(gpu_lib, device=True)


def test_cells_on_the_device(gpu_lib):
    A.cells(gpu_lib, device=True)


def test_strides_on_the_device(gpu_lib):
    A.strides(gpu_lib, device=True)


def test_ref_pose_on_the_device(gpu_lib):
    A.ref_pose(gpu_lib, device=True)


def test_group_on_the_device(gpu_lib):
    A.group(gpu_lib, device=True)


def test_evaluator_matrices_on_the_device(gpu_lib):
    A.evaluator_matrices(gpu_lib, device=True)


def test_wide_group_volume_on_the_device(gpu_lib, oracle):
    A.wide_group(gpu_lib, oracle, device=True)


def test_triclinic_reach_volume_on_the_device(gpu_lib, oracle):
    A.triclinic_reach(gpu_lib, oracle, device=True)
