"""What k_rdf_pencil does outside its column loops - the item queue, the item and chunk prologues, the split-pencil shrink, the choice of the
shifted segment loop - at the edges the cases of segment_table_cases.py do not reach: the same cases for the SIMT emulator build
(test_pencil_walk_emu.py) and the product library on the device (test_pencil_walk_gpu.py).  u64 counts are compared bit for bit with the
oracle's all-pairs evaluation (cases.check_rdf); every case also asserts that the pencil kernel, and not the all-pairs kernel, served it.

Where that code can go wrong: a neighbour reach that differs between y and z (the shrink and the pencil widths it needs exist only when
one of them exceeds 1, and each axis shrinks by its own width), pencil widths of a cell that changes from frame to frame (they belong to the
frame, not to the launch), more frames than frame queues (tickets wrap within a queue, waves steal from the other seven), forced item
counts per pencil (several chunks per item, one, and more items than chunks: items that find no chunk), and chunks whose segments are partly
periodic images and partly not (the segment loop without the shift is chosen from the bit patterns of sx, sy, sz: both zeros are zero)."""
import numpy as np

import cases
import segment_table_cases as S
from viamd_amd import _lib as L


def _reach(O):
    return S._cloud(21, 52.0, 3000), 52.0, L.PBC_ALL, S._sets(3000)


def _ten_frames(O):
    return S._cloud(22, 25.0, 1500, frames=10), 25.0, L.PBC_ALL, S._sets(1500)


def _images_meet(O):
    """2 x 2 pencils of 13 A (r = 12): every neighbour pencil is met as itself and as its image in y, in z and in both; half of the atoms sit
    in a slab around x = 0 = Lx, so that the chunks there have segments of all three x images next to unshifted ones; a few atoms lie
    exactly on the faces"""
    rng = np.random.default_rng(23)
    n = 1600
    c = rng.uniform(0.0, 26.0, (3, 3, n))
    c[:, 0, : n // 2] = np.mod(rng.uniform(-3.0, 3.0, (3, n // 2)), 26.0)
    c[:, :, :6] = np.array([0.0, 26.0, 13.0])[None, :, None] * np.ones((3, 1, 6))
    c[:, 1, 6:12] = 0.0
    c[:, 2, 12:18] = 26.0
    return c.astype(np.float32), 26.0, L.PBC_ALL, S._sets(n)


# name -> (system, options): options are set through vmd_set_option for the case and restored after it
CASES = {
    "reach_2_in_y_1_in_z": (_reach, {"pencil_split_y": 2, "pencil_split_z": 1}),
    "reach_1_in_y_4_in_z": (_reach, {"pencil_split_y": 1, "pencil_split_z": 4}),
    "split_2x2_cell_changes_every_frame": (S._cell_per_frame, {"pencil_split_y": 2, "pencil_split_z": 2}),
    "ten_frames_eight_queues": (_ten_frames, {}),
    "dense_blob_nsub_1": (S._dense, {"rdf_nsub": 1}),
    "dense_blob_nsub_3": (S._dense, {"rdf_nsub": 3}),
    "dense_blob_nsub_64": (S._dense, {"rdf_nsub": 64}),
    "images_meet_unshifted": (_images_meet, {}),
    "images_meet_unshifted_wave_private_hist": (_images_meet, {"rdf_shared_hist": 0}),
}


def run(lib, O, name, device):
    system, options = CASES[name]
    coords, box, flags, props = system(O)
    options = {"rdf_shared_hist": 1, "pencil_split_y": 1, "pencil_split_z": 1, "rdf_nsplit": -1, "rdf_nsub": 0, **options}
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
