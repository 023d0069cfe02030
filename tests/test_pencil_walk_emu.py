"""k_rdf_pencil outside its column loops (item queue, prologues, shrink, shift test) on the SIMT emulator (CPU suite):
tests/pencil_walk_cases.py has the cases."""
import pytest

import pencil_walk_cases as P


@pytest.mark.parametrize("name", list(P.CASES))
def test_pencil_walk(emu_lib, oracle, name):
    P.run(emu_lib, oracle, name, device=False)
