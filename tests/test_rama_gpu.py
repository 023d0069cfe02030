"""Backbone phi / psi and the Ramachandran density on the MI355X: the bodies of tests/test_rama.py through the product
library.  On the device the table follows the rule of test_geometry.check_values (every value within 1 fp32 ulp of the restatement, at
most max(1, size // 1000) values not bit-identical, the count printed); everything integer is exact."""
import pytest

import test_rama as TR

pytestmark = pytest.mark.gpu


def test_known_answers_on_the_device(gpu_lib):
    TR.known_answers(gpu_lib, device=True)
    TR.known_answers(gpu_lib)


@pytest.mark.parametrize("box,tilt,flags", TR.CELLS)
def test_size_edges_on_the_device(gpu_lib, box, tilt, flags):
    TR.size_edges(gpu_lib, box, tilt, flags, exact=False, device=True)


def test_pin_to_dihedral_on_the_device(gpu_lib):
    TR.dihedral_pin(gpu_lib, device=True)
    TR.dihedral_pin(gpu_lib)


def test_map_on_the_device(gpu_lib):
    TR.map_checks(gpu_lib, device=True)


def test_filtered_map_on_the_device(gpu_lib):
    TR.filtered_map(gpu_lib, device=True)
    TR.filtered_map(gpu_lib)


def test_call_patterns_on_the_device(gpu_lib):
    TR.call_patterns(gpu_lib, device=True)
    TR.call_patterns(gpu_lib)


def test_nothing_else_moves_on_the_device(gpu_lib, oracle):
    TR.nothing_else_moves(gpu_lib, oracle, device=True)
