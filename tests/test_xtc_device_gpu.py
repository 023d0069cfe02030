"""The cases of tests/xtc_device_cases.py on the MI355X (device memory from torch): what the emulator cannot show - the ballots, readlanes
and ds_bpermutes of k_xtc_wave and k_xtc_records with 64 lanes at once, the real grids of the frame-per-thread and chunk kernels, and
stores outside a frame's rows, which nothing else would notice on the hardware."""
import pytest

import xtc_device_cases as X

pytestmark = pytest.mark.gpu

_V = pytest.mark.parametrize("chunk", [c for _, c in X.VARIANTS], ids=[n for n, _ in X.VARIANTS])
_V2 = pytest.mark.parametrize("chunk", [c for _, c in X.TWO_PASS], ids=[n for n, _ in X.TWO_PASS])


@_V
@pytest.mark.parametrize("kind,n", X.ATOM_EDGES, ids=[f"{k}{n}" for k, n in X.ATOM_EDGES])
def test_atom_count_edges_on_the_device(gpu_lib, tmp_path, kind, n, chunk):
    X.atom_count_edge(gpu_lib, kind, n, chunk, True, tmp_path if chunk == -3 else None)


def test_chunked_decode_past_64_chunks_on_the_device(gpu_lib):
    X.chunked_past_64_chunks(gpu_lib, True)


@_V
@pytest.mark.parametrize("kind,n,B", X.B_EDGES, ids=[f"{k}{n}x{B}" for k, n, B in X.B_EDGES])
def test_batch_edges_on_the_device(gpu_lib, kind, n, B, chunk):
    X.batch_edge(gpu_lib, kind, n, B, chunk, True)


@_V2
def test_fewer_waves_than_sections_on_the_device(gpu_lib, chunk):
    X.fewer_waves_than_sections(gpu_lib, chunk, True)


@_V
@pytest.mark.parametrize("kind,n,precision", X.PRECISIONS, ids=[f"{k}{n}p{p:g}" for k, n, p in X.PRECISIONS])
def test_precisions_on_the_device(gpu_lib, kind, n, precision, chunk):
    X.precision_case(gpu_lib, kind, n, precision, chunk, True)


@pytest.mark.parametrize("natoms", X.F32_SHAPES)
def test_raw_f32_layouts_on_the_device(gpu_lib, natoms):
    X.raw_f32_case(gpu_lib, natoms, True)
