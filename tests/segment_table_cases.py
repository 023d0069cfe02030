"""The neighbour segment table of k_rdf_pencil at its edges: the same cases for the SIMT emulator build (test_segment_table_emu.py) and the
product library on the device (test_segment_table_gpu.py).  u64 counts are compared bit for bit with the oracle's all-pairs evaluation
(cases.check_rdf); every case also asserts that the pencil kernel, and not the all-pairs kernel, served it.

The table can only go wrong where the combo enumeration, the rounds of combo lanes, the ballots or the own-pencil entry meet an edge:
few pencils (two entries that name the same pencil under different images), more combos than lanes, every cell kind, the part filter of
split launches, empty pencils and partial chunks, several chunks per pencil."""
import numpy as np

import cases
from viamd_amd import _lib as L


def _cloud(seed, box, n, frames=2, spill=0.0):
    """uniform atoms in an orthorhombic box (edges `box`), a few of them outside the cell when spill > 0"""
    rng = np.random.default_rng(seed)
    e = np.array((box,) * 3 if np.isscalar(box) else box[:3], np.float64)
    return (rng.uniform(-spill, 1.0 + spill, (frames, 3, n)) * e[None, :, None]).astype(np.float32)


def _sets(n):
    """a same-set and a two-set property, r = 12: half shell with the own pencil / full shell"""
    a, b = np.arange(0, n, 2, dtype=np.int32), np.arange(1, n, 2, dtype=np.int32)
    return [("gaa", a, a, 0.0, 12.0), ("gab", a, b, 0.0, 12.0)]


def _pencils_2x2(O):
    return _cloud(1, 25.0, 1500), 25.0, L.PBC_ALL, _sets(1500)


def _pencils_3x3(O):
    return _cloud(2, 40.0, 3000), 40.0, L.PBC_ALL, _sets(3000)


def _noncubic(O):
    return _cloud(3, (25.0, 40.0, 61.0), 3000, spill=0.2), (25.0, 40.0, 61.0), L.PBC_ALL, _sets(3000)


def _cell_per_frame(O):
    boxes = [40.0, 42.5, (38.7, 41.0, 44.0)]
    c = np.concatenate([_cloud(4 + f, b, 2400, frames=1) for f, b in enumerate(boxes)])
    return c, boxes, L.PBC_ALL, _sets(2400)


def _sheared(O):
    box = (52.0, 50.0, 49.0, 6.0, -4.0, 5.0)
    A = np.array([[box[0], box[3], box[4]], [0, box[1], box[5]], [0, 0, box[2]]])
    rng = np.random.default_rng(8)
    c = np.einsum("ij,fjn->fin", A, rng.uniform(-0.2, 1.2, (2, 3, 3000))).astype(np.float32)
    return c, box, L.PBC_ALL, _sets(3000)


def _no_cell(O):
    rng = np.random.default_rng(9)
    c = np.stack([rng.normal(0, 14.0 + 2 * f, (3, 2400)) + np.array([[5.0 * f], [-30.0], [100.0]]) for f in range(2)]).astype(np.float32)
    return c, None, L.PBC_ALL, _sets(2400)


def _slab(O):
    c, _, _, props = _no_cell(O)
    return c, (40.0, 36.0, 50.0), 3, props          # periodic in x and y, open along z


def _sparse(O):
    return _cloud(10, 40.0, 200), 40.0, L.PBC_ALL, _sets(200)


def _dense(O):
    """3 x 3 pencils of 13.3 A: a blob of 900 atoms in one pencil (several chunks per pencil), exactly 64 and exactly 65 atoms of each set
    in two others (a full chunk; a full chunk and a one-atom chunk), a thin background"""
    rng = np.random.default_rng(11)
    w = 40.0 / 3.0

    def pencil(py, pz, n, x0=0.0, x1=40.0):
        return np.stack([rng.uniform(x0, x1, (2, n)), rng.uniform(py * w + 0.5, (py + 1) * w - 0.5, (2, n)),
                         rng.uniform(pz * w + 0.5, (pz + 1) * w - 0.5, (2, n))], axis=1)

    c = np.concatenate([pencil(2, 2, 900, 10.0, 20.0), pencil(0, 0, 128), pencil(1, 1, 130), pencil(0, 2, 42), pencil(2, 0, 40)], axis=2)
    return c.astype(np.float32), 40.0, L.PBC_ALL, _sets(c.shape[2])


# name -> (system, options): options are set through vmd_set_option for the case and restored after it
CASES = {
    "2x2_pencils": (_pencils_2x2, {}),
    "2x2_pencils_wave_private_hist": (_pencils_2x2, {"rdf_shared_hist": 0}),
    "3x3_pencils": (_pencils_3x3, {}),
    "3x3_pencils_wave_private_hist": (_pencils_3x3, {"rdf_shared_hist": 0}),
    "split_2x2_25_combos": (_pencils_3x3, {"pencil_split_y": 2, "pencil_split_z": 2}),
    "split_4x4_81_combos": (lambda O: (_cloud(12, 52.0, 3000), 52.0, L.PBC_ALL, _sets(3000)), {"pencil_split_y": 4, "pencil_split_z": 4}),
    "noncubic_25_40_61": (_noncubic, {}),
    "cell_changes_every_frame": (_cell_per_frame, {}),
    "sheared": (_sheared, {}),
    "sheared_split_4x4": (_sheared, {"pencil_split_y": 4, "pencil_split_z": 4}),       # 81 combos on the 32 combo lanes of a triclinic cell
    "no_cell": (_no_cell, {}),
    "slab_xy": (_slab, {}),
    "nsplit_5": (_pencils_3x3, {"rdf_nsplit": 5}),
    "nsplit_9": (_pencils_3x3, {"rdf_nsplit": 9}),
    "nsplit_25": (_pencils_3x3, {"rdf_nsplit": 25, "pencil_split_y": 2, "pencil_split_z": 2}),   # one combo per part (two sets)
    "sparse_200_atoms": (_sparse, {}),
    "dense_blob_64_65": (_dense, {}),
}


def run(lib, O, name, device):
    system, options = CASES[name]
    coords, box, flags, props = system(O)
    options = {"rdf_shared_hist": 1, "pencil_split_y": 1, "pencil_split_z": 1, "rdf_nsplit": -1, **options}
    old = {k: lib.vmd_set_option(k.encode(), v) for k, v in options.items()}
    lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
    try:
        cases.check_rdf(lib, O, coords, box, props, flags=flags, device=device, oracle_method="brute")
    finally:
        lib.vmd_profile_enable(False)
        for k, v in old.items():
            lib.vmd_set_option(k.encode(), v)
    n_grid, n_brute = cases._kernel_family(lib)
    assert n_grid > 0 and n_brute == 0, f"{name}: served by the all-pairs kernel ({n_grid} pencil, {n_brute} all-pairs launches)"
