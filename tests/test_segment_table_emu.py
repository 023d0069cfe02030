"""k_rdf_pencil's lane-built neighbour segment table on the SIMT emulator (CPU suite): tests/segment_table_cases.py has the cases."""
import pytest

import segment_table_cases as S


@pytest.mark.parametrize("name", list(S.CASES))
def test_segment_table(emu_lib, oracle, name):
    S.run(emu_lib, oracle, name, device=False)
