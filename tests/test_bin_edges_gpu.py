"""Pair distances on the bin edges of rdf() on the device: the cases of tests/test_bin_edges_emu.py through the product library, with
the inline-assembly pops (vmd_pop_hot, vmd_pop_hot0, vmd_pop_hot2) that only a device run can judge."""
import pytest

import bin_edge_cases as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("route,rname", B.PARAMS)
def test_bin_edges(gpu_lib, route, rname):
    B.run(gpu_lib, rname, route, device=True)
