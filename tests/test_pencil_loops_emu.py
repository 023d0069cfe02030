"""k_rdf_pencil inside its column loops (one-axis image loops, the own pencil's scalar lane mask) on the SIMT emulator (CPU suite):
tests/pencil_loop_cases.py has the cases."""
import pytest

import pencil_loop_cases as P


@pytest.mark.parametrize("name", list(P.CASES))
def test_pencil_loops(emu_lib, oracle, name):
    P.run(emu_lib, oracle, name, device=False)
