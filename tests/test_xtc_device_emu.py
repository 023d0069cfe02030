"""The device trajectory decoders at their size edges on the SIMT emulator (tests/xtc_device_cases.py): the logic of the checkpoint spacing,
the sectioned passes, the block decomposition of the frame-per-thread kernels and k_raw_f32's layouts, coordinate by coordinate against
tests/xtc_ref.py and inside guards.  The emulator runs one lane at a time, so the ballots, readlanes and ds_bpermutes of k_xtc_wave are
only what the device side of the same cases, tests/test_xtc_device_gpu.py, can show.  Nothing is left out here: every case runs through
every variant, as on the GPU."""
import pytest

import xtc_device_cases as X

_V = pytest.mark.parametrize("chunk", [c for _, c in X.VARIANTS], ids=[n for n, _ in X.VARIANTS])
_V2 = pytest.mark.parametrize("chunk", [c for _, c in X.TWO_PASS], ids=[n for n, _ in X.TWO_PASS])


@_V
@pytest.mark.parametrize("kind,n", X.ATOM_EDGES, ids=[f"{k}{n}" for k, n in X.ATOM_EDGES])
def test_atom_count_edges(emu_lib, tmp_path, kind, n, chunk):
    X.atom_count_edge(emu_lib, kind, n, chunk, False, tmp_path if chunk == -3 else None)


def test_chunked_decode_past_64_chunks(emu_lib):
    X.chunked_past_64_chunks(emu_lib, False)


@_V
@pytest.mark.parametrize("kind,n,B", X.B_EDGES, ids=[f"{k}{n}x{B}" for k, n, B in X.B_EDGES])
def test_batch_edges(emu_lib, kind, n, B, chunk):
    X.batch_edge(emu_lib, kind, n, B, chunk, False)


@_V2
def test_fewer_waves_than_sections(emu_lib, chunk):
    X.fewer_waves_than_sections(emu_lib, chunk, False)


@_V
@pytest.mark.parametrize("kind,n,precision", X.PRECISIONS, ids=[f"{k}{n}p{p:g}" for k, n, p in X.PRECISIONS])
def test_precisions(emu_lib, kind, n, precision, chunk):
    X.precision_case(emu_lib, kind, n, precision, chunk, False)


@pytest.mark.parametrize("natoms", X.F32_SHAPES)
def test_raw_f32_layouts(emu_lib, natoms):
    X.raw_f32_case(emu_lib, natoms, False)
