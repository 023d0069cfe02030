"""Per-frame secondary structure on the MI355X: the bodies of tests/test_ss.py through the product library.  Class codes and
populations are integers: the rule on the device is exact equality with the restatement, as on the emulator.  Where a code differs,
test_ss.check prints the segment and, for every bond the restatement evaluated for it, the four distances, the energy and the CA gate."""
import pytest

import test_ss as TS

pytestmark = pytest.mark.gpu


def test_known_answers_on_the_device(gpu_lib):
    TS.known_answers(gpu_lib, device=True)
    TS.known_answers(gpu_lib)


@pytest.mark.parametrize("cell", range(len(TS.CELLS)))
def test_size_edges_on_the_device(gpu_lib, cell):
    TS.size_edges(gpu_lib, cell, device=True)


def test_near_thresholds_on_the_device(gpu_lib):
    TS.near_thresholds(gpu_lib, device=True)
    TS.near_thresholds(gpu_lib)


def test_next_to_the_other_forms_on_the_device(gpu_lib, oracle):
    TS.next_to_the_other_forms(gpu_lib, oracle, device=True)


def test_call_patterns_on_the_device(gpu_lib):
    TS.call_patterns(gpu_lib, device=True)
    TS.call_patterns(gpu_lib)
