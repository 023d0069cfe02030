"""The cell builds at their size edges on the SIMT emulator (tests/cell_build_cases.py): the scans, the stretches of the tables, the slices
and the bucket records of all five builds, cell_start and the sorted copy held bit for bit against the oracle's wrap and a NumPy
restatement of the cell index.  The device side of the same cases is tests/test_cell_build_gpu.py."""
import pytest

import cell_build_cases as D


@pytest.mark.parametrize("build,nsel", D.SINGLE_NSEL)
def test_single_level_selection_sizes(emu_lib, oracle, build, nsel):
    D.single_nsel(emu_lib, oracle, build, nsel)


@pytest.mark.parametrize("build,ncell", D.SINGLE_NCELL)
def test_single_level_table_sizes(emu_lib, oracle, build, ncell):
    D.single_ncell(emu_lib, oracle, build, ncell)


@pytest.mark.parametrize("build", ("atomic", "fused", "split"))
def test_single_level_index_list_forms_and_an_open_axis(emu_lib, oracle, build):
    D.single_forms(emu_lib, oracle, build)


@pytest.mark.parametrize("nsel", D.PENCIL_NSEL)
def test_two_level_selection_sizes(emu_lib, oracle, nsel):
    D.pencil_nsel(emu_lib, oracle, nsel)


@pytest.mark.parametrize("npen", D.PENCIL_NPEN)
def test_two_level_pencil_counts(emu_lib, oracle, npen):
    D.pencil_npen(emu_lib, oracle, npen)


@pytest.mark.parametrize("nxf", D.PENCIL_NXF)
def test_two_level_fine_cells_per_pencil(emu_lib, oracle, nxf):
    D.pencil_nxf(emu_lib, oracle, nxf)


@pytest.mark.parametrize("lds,rec3", D.COMBOS)
def test_two_level_index_list_forms_and_open_axes(emu_lib, oracle, lds, rec3):
    D.pencil_forms(emu_lib, oracle, lds, rec3)


@pytest.mark.parametrize("lds,rec3", D.COMBOS)
def test_two_level_overflow_raises_the_threads_bit(emu_lib, oracle, lds, rec3):
    D.pencil_overflow(emu_lib, oracle, lds, rec3)
