"""k_rdf_pencil's lane-built neighbour segment table on the device: the cases of the emulator file (tests/segment_table_cases.py) through
the product library, trajectory resident in device memory."""
import pytest

import segment_table_cases as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(S.CASES))
def test_segment_table(gpu_lib, oracle, name):
    S.run(gpu_lib, oracle, name, device=True)
