"""Targets on the voxel faces of sdf() on the device: the cases of tests/test_voxel_faces_emu.py through the product library."""
import pytest

import voxel_face_cases as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(F.CASES))
@pytest.mark.parametrize("route", list(F.ROUTES))
def test_voxel_faces(gpu_lib, route, name):
    F.run(gpu_lib, name, route, device=True)


@pytest.mark.parametrize("n", F.SIZES)
def test_counts_to_float(gpu_lib, n):
    F.counts_to_float(gpu_lib, n, device=True)


@pytest.mark.parametrize("n", F.SIZES)
def test_axpy_and_add_u64(gpu_lib, n):
    F.axpy_add(gpu_lib, n, device=True)
