"""Pair distances on the bin edges of rdf() (tests/bin_edge_cases.py) through the SIMT emulator build: vmd_bin_add, the C++ twins of the
pops, vmd_bin_of and the all-pairs kernels against tests/rdf_ref.py, count for count.  The inline-assembly pops are not in this build:
tests/test_bin_edges_gpu.py runs the same cases on the device."""
import pytest

import bin_edge_cases as B


@pytest.mark.parametrize("route,rname", B.PARAMS)
def test_bin_edges(emu_lib, route, rname):
    B.run(emu_lib, rname, route)
