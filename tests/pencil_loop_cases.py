"""What k_rdf_pencil does inside its column loops for the two kinds of columns that are not the plain ones: columns of periodic images (the
shifted segment loops: one subtraction per live shift axis, the general loop for the rest; `rdf_shift_axes` = 0 sends every shifted segment
through the general loop) and columns of a chunk's own pencil (the j > i mask, made on the scalar unit from j - cbeg).  The same cases for the
SIMT emulator build (test_pencil_loops_emu.py) and the product library on the device (test_pencil_loops_gpu.py).  u64 counts are compared
bit for bit with the oracle's all-pairs evaluation (cases.check_rdf); every case also asserts that the pencil kernel, and not the all-pairs
kernel, served it.  A shift case is evaluated a second time with `rdf_shift_axes` = 0 and must give the same counts.

Where that code can go wrong: a segment whose only live axis is taken for another one (edges that differ, so the wrong shift changes counts),
segments with two live axes (y and z wrapped; a triclinic cell, where sx moves with sy and sz) taking a one-axis loop, an image invented on an
open axis; a mask one lane too wide or too narrow (the j = cbeg column passes no lane, the last column of a full chunk 63), a ragged last
chunk, a second chunk of the same pencil, a stack that fills up inside the masked loop, the columns past a segment's end in its last group.

What no count can show: a mask ONE lane too wide.  The extra lane of column j is lane j - cbeg, the atom against itself, d2 = 0, which the open
interval at 0 (and any r_min) rejects behind the stack.  One lane too narrow, or two too wide, changes the populations' counts.

Not here: a shift of -0.0.  The front-end cannot make one - sy / sz are a literal 0 or +-L of a positive edge, an x image's zero carries the
sign of Lx, a triclinic cell's sums start from +0 - and a periodic edge of -0.0 has no pencil grid (the all-pairs kernel serves it)."""
import numpy as np

import cases
import segment_table_cases as S
import viamd_amd as V
from viamd_amd import _lib as L


def _slab_cloud(seed, edges, n, frames=2):
    """uniform atoms in an orthorhombic cell; half of them in a slab around x = 0 = Lx, so that the chunks there have segments of all three x
    images next to unshifted ones; a few atoms exactly on the faces"""
    rng = np.random.default_rng(seed)
    e = np.array(edges, np.float64)
    c = rng.uniform(0.0, 1.0, (frames, 3, n)) * e[None, :, None]
    c[:, 0, : n // 2] = np.mod(rng.uniform(-3.0, 3.0, (frames, n // 2)), e[0])
    c[:, :, :6] = np.array([0.0, e[1], e[2] / 2])[None, :, None] * np.ones((frames, 1, 6))
    c[:, 0, 6:12] = e[0]
    c[:, 1, 12:18] = 0.0
    c[:, 2, 18:24] = e[2]
    return c.astype(np.float32)


def _cube_39(O):
    """3 x 3 pencils of 13 A (r = 12): every chunk meets neighbours wrapped in y only, in z only, in both and in neither"""
    return _slab_cloud(31, (39.0,) * 3, 2400), 39.0, L.PBC_ALL, S._sets(2400)


def _edges_40_27_53(O):
    """2 pencils in y, 4 in z, three different edges: the shift of the wrong axis changes counts"""
    return _slab_cloud(32, (40.0, 27.0, 53.0), 2400), (40.0, 27.0, 53.0), L.PBC_ALL, S._sets(2400)


def _sheared(O, box, seed):
    A = np.array([[box[0], box[3], box[4]], [0, box[1], box[5]], [0, 0, box[2]]])
    rng = np.random.default_rng(seed)
    c = np.einsum("ij,fjn->fin", A, rng.uniform(-0.2, 1.2, (2, 3, 2400))).astype(np.float32)
    return c, box, L.PBC_ALL, S._sets(2400)


def _triclinic(O):
    """sx is live together with sy or sz: those segments go the general way"""
    return _sheared(O, (52.0, 50.0, 49.0, 6.0, -4.0, 5.0), 33)


def _triclinic_yz_only(O):
    """a triclinic cell whose x does not move with y or z: a y-wrapped neighbour has sy alone, a z-wrapped one sy (= +-yz) and sz"""
    return _sheared(O, (44.0, 42.0, 40.0, 0.0, 0.0, 5.0), 34)


def _partly(flags):
    def system(O):
        rng = np.random.default_rng(35 + flags)
        c = np.stack([rng.normal(0, 13.0 + 2 * f, (3, 2400)) + np.array([[5.0 * f], [-30.0], [100.0]]) for f in range(2)]).astype(np.float32)
        return c, (40.0, 36.0, 50.0), flags, S._sets(2400)
    return system


POPULATIONS = (1, 2, 63, 64, 65, 127, 128, 130)


def _blob(rng, n, frames=2):
    """n atoms inside one pencil of the 39 A cube (the middle one), within r / 2 = 6 A of each other: every admissible pair is a hit"""
    return 19.5 + rng.uniform(-1.7, 1.7, (frames, 3, n))


def _populations(rmin):
    def system(O):
        rng = np.random.default_rng(41)
        c = np.concatenate([_blob(rng, n) for n in POPULATIONS], axis=2).astype(np.float32)
        props, at = [], 0
        for n in POPULATIONS:
            sel = np.arange(at, at + n, dtype=np.int32)
            props.append((f"g{n}", sel, sel, rmin, 12.0))
            at += n
        return c, 39.0, L.PBC_ALL, props
    return system


def _coincident(O):
    """70 atoms in one pencil; two of them coincide (d2 = 0: never counted), two are exactly r_max apart along the pencil (open interval)"""
    rng = np.random.default_rng(42)
    c = _blob(rng, 70)
    c[:, :, 1] = c[:, :, 0]
    c[:, :, 2] = np.array([10.0, 19.5, 19.5])[None, :]
    c[:, :, 3] = np.array([22.0, 19.5, 19.5])[None, :]
    sel = np.arange(70, dtype=np.int32)
    return c.astype(np.float32), 39.0, L.PBC_ALL, [("g", sel, sel, 0.0, 12.0)]


# name -> (system, options, both): options are set through vmd_set_option for the case and restored after it; both: evaluated with
# rdf_shift_axes = 1 (against the oracle) and = 0 (against the first evaluation)
CASES = {
    "cube_39_3x3_pencils": (_cube_39, {}, True),
    "cube_39_wave_private_hist": (_cube_39, {"rdf_shared_hist": 0}, True),
    "edges_40_27_53": (_edges_40_27_53, {}, True),
    "triclinic": (_triclinic, {}, True),
    "triclinic_yz_only": (_triclinic_yz_only, {}, True),
    "periodic_x_only": (_partly(1), {}, True),
    "periodic_y_only": (_partly(2), {}, True),
    "dense_blob_nsub_1": (S._dense, {"rdf_nsub": 1}, True),
    "dense_blob_nsub_3": (S._dense, {"rdf_nsub": 3}, True),
    "own_pencil_populations": (_populations(0.0), {}, False),
    "own_pencil_populations_wave_private_hist": (_populations(0.0), {"rdf_shared_hist": 0}, False),
    "own_pencil_populations_r_min": (_populations(0.75), {}, False),
    "own_pencil_coincident_and_r_max": (_coincident, {}, False),
}


def _counts(lib, O, coords, box, flags, props, device):
    """the evaluator's integer histograms alone, name -> u64[1024]"""
    _, vcell = cases.cell_pair(O, box, flags)
    ir = V.ScriptIR(lib)
    for name, ref, tgt, rmin, rmax in props:
        ir.add_rdf(name, ref, tgt, (rmin, rmax))
    F, _, N = coords.shape
    ev = V.ScriptEval(F, ir)
    traj = cases.make_traj(lib, coords, vcell, device)
    assert ev.frame_range(V.MolSystem(N, unitcell=vcell), traj, 0, F)
    return {name: np.array(ev.property_data(name).counts, copy=True) for name, *_ in props}


def run(lib, O, name, device):
    system, options, both = CASES[name]
    coords, box, flags, props = system(O)
    options = {"rdf_shared_hist": 1, "pencil_split_y": 1, "pencil_split_z": 1, "rdf_nsplit": -1, "rdf_nsub": 0, "rdf_shift_axes": 1, **options}
    old = {k: lib.vmd_set_option(k.encode(), v) for k, v in options.items()}
    assert old["rdf_shift_axes"] == 1, "rdf_shift_axes is on by default"
    lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
    try:
        ev = cases.check_rdf(lib, O, coords, box, props, flags=flags, device=device, oracle_method="brute")
        if both:
            first = {name_: np.array(ev.property_data(name_).counts, copy=True) for name_, *_ in props}
            assert lib.vmd_set_option(b"rdf_shift_axes", 0) == 1
            second = _counts(lib, O, coords, box, flags, props, device)
            for k in first:
                np.testing.assert_array_equal(second[k], first[k], err_msg=f"{name} / {k}: rdf_shift_axes = 0 and 1 count differently")
    finally:
        lib.vmd_profile_enable(False)
        for k, v in old.items():
            lib.vmd_set_option(k.encode(), v)
    n_grid, n_brute = cases._kernel_family(lib)
    assert n_grid > 0 and n_brute == 0, f"{name}: served by the all-pairs kernel ({n_grid} pencil, {n_brute} all-pairs launches)"
    if name.startswith("own_pencil_populations") and props[0][3] == 0.0:
        # every admissible pair is a hit - the sum of the counts is known without the oracle: 2 per unordered pair and frame
        for (pname, *_), n in zip(props, POPULATIONS):
            assert int(ev.property_data(pname).counts.sum()) == coords.shape[0] * n * (n - 1), pname
