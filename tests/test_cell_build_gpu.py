"""The cases of tests/cell_build_cases.py on the MI355X, from buffers in device memory: what the emulator cannot show - the block scans'
barriers, the wave-barrier scan of k_cells_bin_sorted and the LDS and global atomics on real waves, the real LDS opt-in."""
import pytest

import cell_build_cases as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("build,nsel", D.SINGLE_NSEL)
def test_single_level_selection_sizes_on_the_device(gpu_lib, oracle, build, nsel):
    D.single_nsel(gpu_lib, oracle, build, nsel, gpu=True)


@pytest.mark.parametrize("build,ncell", D.SINGLE_NCELL)
def test_single_level_table_sizes_on_the_device(gpu_lib, oracle, build, ncell):
    D.single_ncell(gpu_lib, oracle, build, ncell, gpu=True)


@pytest.mark.parametrize("build", ("atomic", "fused", "split"))
def test_single_level_index_list_forms_and_an_open_axis_on_the_device(gpu_lib, oracle, build):
    D.single_forms(gpu_lib, oracle, build, gpu=True)


@pytest.mark.parametrize("nsel", D.PENCIL_NSEL)
def test_two_level_selection_sizes_on_the_device(gpu_lib, oracle, nsel):
    D.pencil_nsel(gpu_lib, oracle, nsel, gpu=True)


@pytest.mark.parametrize("npen", D.PENCIL_NPEN)
def test_two_level_pencil_counts_on_the_device(gpu_lib, oracle, npen):
    D.pencil_npen(gpu_lib, oracle, npen, gpu=True)


@pytest.mark.parametrize("nxf", D.PENCIL_NXF)
def test_two_level_fine_cells_per_pencil_on_the_device(gpu_lib, oracle, nxf):
    D.pencil_nxf(gpu_lib, oracle, nxf, gpu=True)


@pytest.mark.parametrize("lds,rec3", D.COMBOS)
def test_two_level_index_list_forms_and_open_axes_on_the_device(gpu_lib, oracle, lds, rec3):
    D.pencil_forms(gpu_lib, oracle, lds, rec3, gpu=True)


@pytest.mark.parametrize("lds,rec3", D.COMBOS)
def test_two_level_overflow_raises_the_threads_bit_on_the_device(gpu_lib, oracle, lds, rec3):
    D.pencil_overflow(gpu_lib, oracle, lds, rec3, gpu=True)
