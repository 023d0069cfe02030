"""The SDF scatter kernels at their size edges on the SIMT emulator (tests/sdf_scatter_cases.py): the logic of the target addressing, the
group test's bit mask, the per-block and per-wave rounds and the persistent walk, against the oracle count for count.  The device side of
the same cases is tests/test_sdf_scatter_gpu.py.

No case of the device list is left out: the two largest (4 097 targets at 8 / 16 per thread, the 129-tile walk of the streaming kernel
over 11 008 targets x 3 frames) take the emulator about a second each."""
import pytest

import sdf_scatter_cases as D


@pytest.mark.parametrize("ntgt", D.TARGET_COUNTS)
def test_target_count_against_the_tiles(emu_lib, oracle, ntgt):
    D.target_count(emu_lib, oracle, ntgt)


@pytest.mark.parametrize("ntgt", D.ILP_COUNTS)
def test_target_count_against_the_tiles_of_8_and_16_per_thread(emu_lib, oracle, ntgt):
    D.ilp_target_count(emu_lib, oracle, ntgt)


@pytest.mark.parametrize("n_near", D.BLOCK_NEAR)
def test_block_rounds(emu_lib, oracle, n_near):
    D.block_rounds(emu_lib, oracle, n_near)


@pytest.mark.parametrize("n_near", D.WAVE_NEAR)
def test_wave_rounds(emu_lib, oracle, n_near):
    D.wave_rounds(emu_lib, oracle, n_near)


@pytest.mark.parametrize("ntgt,frames", D.STREAM_WALKS)
def test_stream_walk(emu_lib, oracle, ntgt, frames):
    D.stream_walk(emu_lib, oracle, ntgt, frames)


def test_rows_shapes(emu_lib, oracle):
    D.rows_shapes(emu_lib, oracle)


def test_dense_shapes(emu_lib, oracle):
    D.dense_shapes(emu_lib, oracle)


def test_seven_structures(emu_lib, oracle):
    D.seven_structures(emu_lib, oracle)


def test_targets_include_the_structures_own_atoms(emu_lib, oracle):
    D.own_atoms(emu_lib, oracle)
