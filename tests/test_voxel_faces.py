"""tests/sdf_voxel_ref.py judged on the CPU, on every case of tests/voxel_face_cases.py: what the cases must hold before anything is
launched, the exact tier with its margin, and the reference against the oracle's scatter voxel for voxel.  Run with -s for the figures."""
import numpy as np
import pytest

import cases
import sdf_voxel_ref as S
import voxel_face_cases as F


@pytest.mark.parametrize("name", list(F.CASES))
def test_conditions_and_exact_tier(name):
    F.conditions(F.case(name))


@pytest.mark.parametrize("name", list(F.CASES))
def test_reference_is_the_oracle(oracle, name):
    cs = F.case(name)
    edges = tuple(float(v) for v in cs.box9[:3])
    ocell, _ = cases.cell_pair(oracle, edges, cs.pbc)
    for include_self in (0, 1):
        old = oracle.set_spec("sdf_include_self", include_self)
        try:
            vol = np.zeros(F.DIM ** 3, np.uint64)
            for b in range(cs.B):
                x = cs.xyz[b, :, :cs.N]
                oracle.sdf_frame_scatter(x[0], x[1], x[2], ocell, cs.structs, cs.R32[b], cs.c32[b], cs.tgt, float(cs.s), F.DIM, vol)
        finally:
            oracle.set_spec("sdf_include_self", old)
        np.testing.assert_array_equal(vol, cs.want(bool(include_self)), err_msg=f"{name}: include_self = {include_self}")


def test_the_rule_at_zero_and_dim():
    """0 <= t < dim: -0.0 is in and lands in voxel 0, the float below 0 and dim itself are out, the float below dim is in voxel 127"""
    z = np.float32(0.0)
    t = np.float32([[-0.0, np.nextafter(z, np.float32(-1)), 128.0, np.nextafter(np.float32(128.0), z), 0.0]] * 3)
    assert S.in_range(t).tolist() == [True, False, False, True, True]
    assert S.voxel(t[:, [0, 3, 4]]).tolist() == [[0, 127, 0]] * 3
    assert float(S.vscale_of(8.0)) == 8.0 and S.vscale_of(10.0) == np.float32(6.4) and S.rho(8.0) == 1 and S.rho(10.0) != 1


def test_rne32():
    for v, want in ((2 ** 24 - 1, 2.0 ** 24 - 1), (2 ** 24 + 1, 2.0 ** 24), (2 ** 24 + 3, 2.0 ** 24 + 4), (2 ** 32 + 1, 2.0 ** 32), (2 ** 53 + 1, 2.0 ** 53),
                    (2 ** 25 + 2, 2.0 ** 25), (2 ** 25 + 6, 2.0 ** 25 + 8), (2 ** 25 + 3, 2.0 ** 25 + 4)):
        assert float(F._rne32(v)) == want, v
    c = np.concatenate([F.SPECIAL, np.arange(2 ** 24 - 4, 2 ** 24 + 9, dtype=np.uint64)])
    np.testing.assert_array_equal(F.to_f32(c), c.astype(np.float32))
