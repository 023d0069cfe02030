"""k_rdf_pencil inside its column loops (one-axis image loops, the own pencil's scalar lane mask) on the device: the cases of the emulator
file (tests/pencil_loop_cases.py) through the product library, trajectory resident in device memory."""
import pytest

import pencil_loop_cases as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(P.CASES))
def test_pencil_loops(gpu_lib, oracle, name):
    P.run(gpu_lib, oracle, name, device=True)
