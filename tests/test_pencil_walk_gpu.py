"""k_rdf_pencil outside its column loops (item queue, prologues, shrink, shift test) on the device: the cases of the emulator file
(tests/pencil_walk_cases.py) through the product library, trajectory resident in device memory."""
import pytest

import pencil_walk_cases as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(P.CASES))
def test_pencil_walk(gpu_lib, oracle, name):
    P.run(gpu_lib, oracle, name, device=True)
