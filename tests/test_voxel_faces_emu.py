"""Targets on the voxel faces of sdf() (tests/voxel_face_cases.py) through the SIMT emulator build: every scatter kernel, direct calls,
against tests/sdf_voxel_ref.py voxel for voxel; and the accumulators' small kernels.  The device side is tests/test_voxel_faces_gpu.py."""
import pytest

import voxel_face_cases as F


@pytest.mark.parametrize("name", list(F.CASES))
@pytest.mark.parametrize("route", list(F.ROUTES))
def test_voxel_faces(emu_lib, route, name):
    F.run(emu_lib, name, route)


@pytest.mark.parametrize("n", F.SIZES)
def test_counts_to_float(emu_lib, n):
    F.counts_to_float(emu_lib, n)


@pytest.mark.parametrize("n", F.SIZES)
def test_axpy_and_add_u64(emu_lib, n):
    F.axpy_add(emu_lib, n)
