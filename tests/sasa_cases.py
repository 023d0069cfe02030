"""The systems of tests/test_sasa.py and tests/test_sasa_gpu.py: small, seeded, built once per process.  The water boxes and
the three cells are those of tests/hbond_cases.py."""
import numpy as np

import hbond_cases as HC

f32 = np.float32
PROBE, NPOINTS = 1.4, 96
R_O, R_H = 1.52, 1.20                   # Bondi
CELLS = HC.CELLS
# one lane, the wave seam, the block seam
NMEAS = [1, 63, 64, 65, 255, 256, 257]
# one entry, the LDS tile's quarter, and the three sizes around shell_brute_below (480), where the route changes
NENV = [1, 64, 65, 479, 480, 481]
# the word seams of the point mask
NPOINTS_EDGES = [1, 31, 32, 33, 63, 64, 65, 96, 128, 129, 255, 256]
# water with the probe: r_cut = 2 (1.52 + 1.4) = 5.84.  choose_grid wants 2.002 r_cut = 11.692 < L on a periodic axis: just large enough
# for a grid, and too small for one (all pairs whatever is asked)
R_CUT = 2.0 * (R_O + PROBE)
TIGHT, TOO_SMALL = 11.8, 11.6


def water_radii(n_w):
    return np.tile(np.array([R_O, R_H, R_H], np.float32), n_w)


def water_lists(n_w):
    """every atom measured against every atom: dict(measured, measured_radius, env, env_radius)"""
    a = np.arange(3 * n_w, dtype=np.int32)
    r = water_radii(n_w)
    return dict(measured=a, measured_radius=r, env=a, env_radius=r)


def subset_lists(n_w, nmeas, nenv, seed):
    """nmeas and nenv of the water box's atoms, two independent draws in shuffled list order (a measured atom may be missing from the
    environment)"""
    rng = np.random.default_rng(seed)
    r = water_radii(n_w)
    i = rng.permutation(3 * n_w)[:nmeas].astype(np.int32)
    j = rng.permutation(3 * n_w)[:nenv].astype(np.int32)
    return dict(measured=i, measured_radius=r[i], env=j, env_radius=r[j])


def mixed_radii_lists(n_w, seed):
    """the water box with one fat environment atom in a hundred (radius 6.0): r_cut = 14.8 is far from the tight bound of most pairs"""
    s = water_lists(n_w)
    r = s["env_radius"].copy()
    r[np.random.default_rng(seed).permutation(r.size)[:max(1, r.size // 100)]] = 6.0
    return dict(s, env_radius=r)
