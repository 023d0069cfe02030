"""distance / distance_min / distance_max / distance_pair at their size edges on the SIMT emulator (tests/distance_cases.py): the logic of
the strided pair loop, the reduction tree, the thread-to-(frame, context) decompositions and ragged offsets, against the oracle bit for
bit and against tests/distance_ref.py.  The device side of the same cases is tests/test_distance_gpu.py."""
import distance_cases as D


def test_minmax_planted_extremum(emu_lib, oracle):
    D.minmax_planted_extremum(emu_lib, oracle)


def test_minmax_pair_count_edges(emu_lib, oracle):
    D.minmax_pair_count_edges(emu_lib, oracle)


def test_ragged_populations(emu_lib, oracle):
    D.ragged_populations(emu_lib, oracle)


def test_com_slots(emu_lib, oracle):
    D.com_slots(emu_lib, oracle)


def test_com_large_set(emu_lib, oracle):
    D.com_large_set(emu_lib, oracle)


def test_pair_populations(emu_lib, oracle):
    D.pair_populations(emu_lib, oracle)


def test_batching(emu_lib, oracle):
    D.batching(emu_lib, oracle)


def test_triclinic(emu_lib, oracle):
    D.triclinic(emu_lib, oracle)


def test_script_level(emu_lib, oracle):
    D.script_level(emu_lib, oracle)


def test_launcher_rejects_more_than_2_31_frame_contexts(emu_lib):
    """B * P is an int inside vmd_hip_distance and sits on grid.x: 65 536 frames x 65 536 contexts must be refused like
    vmd_hip_geometry refuses them, before anything is launched (every pointer here is null)"""
    hipErrorInvalidValue = 1
    for kind in (0, 1, 2, 3):
        rc = emu_lib.vmd_hip_distance(None, None, 0, 0, None, 7, 65536, kind, 65536, 1, None, None, None, None, None, None, None)
        assert rc == hipErrorInvalidValue, (kind, rc)
    # an empty batch is still nothing to do, not an error
    assert emu_lib.vmd_hip_distance(None, None, 0, 0, None, 7, 0, 0, 65536, 1, None, None, None, None, None, None, None) == 0
