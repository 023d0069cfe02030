"""Writes ref_pin.npz: the outputs of the reference's own histogram functions (oracle/_ref/libviamd_ref.so, compiled by
oracle/make_ref.py from the reference's sources) on the inputs of tests/test_ref_pin.py, so that the tests hold the oracle and the
product against the reference without its sources.  Run: python tests/golden/make_ref_pin.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

import conftest  # noqa: E402
import test_ref_pin as T  # noqa: E402
from oracle import oracle as O  # noqa: E402
from viamd_amd import VmdLib  # noqa: E402


def main():
    lib = T.load_ref_lib()
    if lib is None:
        raise SystemExit("the compiled reference is not available (oracle/make_ref.py needs the reference's sources)")
    O.build()
    O.lib()
    emu = VmdLib(conftest.build_emu())
    record = {}
    for test in (T.test_compute_histogram_against_the_reference, T.test_compute_histogram_masked_against_the_reference,
                 T.test_downsample_and_scale_against_the_reference, T.test_g_of_r_of_an_evaluated_rdf_through_the_reference_downsample):
        test(T.Ref(test.__name__, lib, None, record), O, emu)      # the test's own assertions run against the reference's live outputs
    np.savez_compressed(T.GOLDEN, **record)
    print(f"{T.GOLDEN}: {len(record)} outputs")


if __name__ == "__main__":
    main()
