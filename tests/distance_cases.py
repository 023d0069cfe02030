"""The distance kernels at their size edges: the same cases for the SIMT emulator build (test_distance_emu.py) and the product library on
the device (test_distance_gpu.py).  Every case goes through ScriptIR.add_distance / add_distance_population, ScriptEval.frame_range and
the C ABI, and asserts both bit-equality with the oracle (cases.check_distances) and the comparison with tests/distance_ref.py: the
restatement bit for bit for distance(), plain fp64 within 16 * 2^-24 * max(L, |x|) for distance_min / _max / _pair.

What the small tests never reach: a second trip through the strided pair loop of k_distance_minmax and real values on every level of
its LDS reduction, a second block of k_distance_com, ragged context offsets, a pair population with gridDim.y > 1, batch boundaries."""
import numpy as np

import cases
import distance_ref as R
from viamd_amd import _lib as L
from viamd_amd import script, synth

KIND = {"distance": L.DIST_COM, "distance_min": L.DIST_MIN, "distance_max": L.DIST_MAX, "distance_pair": L.DIST_PAIR}
TRICLINIC = (50.0, 50.0, 50.0, 12.0, -8.0, 10.0)


def rows(ev, name):
    pd = ev.property_data(name)
    return pd.values.reshape(pd.dim[0], -1).copy()


def _is_tri(box):
    return box is not None and not np.isscalar(box) and len(box) == 6 and any(box[3:])


def compare_ref(ev, coords, box, mass, specs, flags, what, geometric=False):
    """every value of every property against distance_ref; prints and returns the largest deviation from the fp64 layer in units of
    2^-24 * M.  Triclinic MIN / MAX / PAIR have no plain reference (the image rule is discontinuous): the oracle alone checks them."""
    worst = 0.0
    for sp in specs:
        name, a, b, kind = sp[:4]
        a_sets, b_sets = (a, b) if len(sp) == 5 else ([a], [b])
        got = rows(ev, name)
        if kind == L.DIST_COM:
            ref = R.com(coords, box, a_sets, b_sets, mass, flags=flags, geometric=geometric)
            assert got.shape == ref.shape, (what, name, got.shape, ref.shape)
            np.testing.assert_array_equal(got.view(np.int32), ref.view(np.int32), err_msg=f"{what} {name}: differs from the restatement")
            print(f"{what} {name}: {got.size} values bit-identical to the restatement")
            continue
        if _is_tri(box):
            continue
        if kind == L.DIST_PAIR:
            ref = np.concatenate([R.pair(coords, box, flags, x, y) for x, y in zip(a_sets, b_sets)], axis=1)
        else:
            ref = np.stack([R.minmax(coords, box, flags, x, y, kind == L.DIST_MAX) for x, y in zip(a_sets, b_sets)], axis=1)
        u = R.units(got, ref, coords, box)
        print(f"{what} {name}: {got.size} values, max deviation {u.max():.2f} units of 2^-24 M from the fp64 reference")
        assert u.max() <= R.UNITS, f"{what} {name}: {u.max():.2f} units of 2^-24 M from the fp64 reference"
        worst = max(worst, float(u.max()))
    return worst


def check(lib, O, coords, box, mass, specs, what, flags=L.PBC_ALL, device=False, ranges=None, geometric=False, **kw):
    ev = cases.check_distances(lib, O, coords, box, mass, specs, flags=flags, device=device, ranges=ranges, **kw)
    worst = compare_ref(ev, coords, box, mass, specs, flags, what, geometric)
    return ev, worst


class _options:
    """library options for the length of a case, restored afterwards"""

    def __init__(self, lib, **opts):
        self.lib, self.opts = lib, opts

    def __enter__(self):
        self.old = {k: self.lib.vmd_set_option(k.encode(), v) for k, v in self.opts.items()}

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.lib.vmd_set_option(k.encode(), v)


# ---- k_distance_minmax: a planted extremum at chosen (thread, trip) ------------------------------------------------------------------

NA, NB = 300, 41        # 12 300 pairs = 48 full trips of 256 threads + 12 threads of a 49th
# (k mod 256, k div 256) of the planted pair, one per frame: thread 0; the last lane of the first wave; the first of the second; the
# levels o = 64 and o = 128 of the reduction; the last thread; the ragged tail; first, middle and last trip
PLANTS = [(0, 0), (63, 0), (64, 1), (127, 47), (128, 1), (255, 47), (11, 48), (200, 47)]


def _lattices():
    """a: 10 x 10 x 3 sites 3 A apart; b: 41 sites of a 7 x 7 plane 20 A above it; the atoms of both in shuffled index order"""
    ga = np.array([(3.0 * i, 3.0 * j, 3.0 * k) for k in range(3) for j in range(10) for i in range(10)], np.float32)
    gb = np.array([(3.0 * i, 3.0 * j, 26.0) for j in range(7) for i in range(7)], np.float32)[:NB]
    perm = np.random.default_rng(41).permutation(NA + NB).astype(np.int32)
    return ga, gb, perm[:NA], perm[NA:]


def _planted(mode):
    """-> coords [8, 3, 341], a, b.  mode "min": b[ib*] sits 1.25 A beside a[ia*] (the next a site is 1.75 A away: 1.25 is the unique
    minimum, and exact in fp32); "max": the pair sits at x = -500 and +500 (1 000 A, every other pair below 540); "min_pbc": the "min"
    plant in a cube of 64 A with the whole system shifted so that a[ia*] is at x = 63.5 and b[ib*] at 64.75, which wraps to 0.75"""
    ga, gb, a, b = _lattices()
    coords = np.zeros((len(PLANTS), 3, NA + NB), np.float32)
    for f, (r, t) in enumerate(PLANTS):
        k = r + 256 * t
        assert k < NA * NB
        ia, ib = divmod(k, NB)
        xa, xb = ga.copy(), gb.copy()
        if mode == "max":
            xa[ia] = (-500.0, 0.0, 0.0); xb[ib] = (500.0, 0.0, 0.0)
        else:
            xb[ib] = xa[ia] + np.array((1.25, 0.0, 0.0), np.float32)
        if mode == "min_pbc":
            shift = np.float32(63.5) - xa[ia, 0]
            xa[:, 0] += shift; xb[:, 0] += shift
        coords[f][:, a] = xa.T
        coords[f][:, b] = xb.T
    return coords, a, b


def minmax_planted_extremum(lib, O, device=False):
    mass = np.ones(NA + NB, np.float32)
    worst = 0.0
    for mode, box, name, want in (("min", None, "mn", 1.25), ("max", None, "mx", 1000.0), ("min_pbc", 64.0, "mn", 1.25)):
        coords, a, b = _planted(mode)
        ev, w = check(lib, O, coords, box, mass, [("mn", a, b, L.DIST_MIN), ("mx", a, b, L.DIST_MAX)], f"planted {mode}", device=device)
        got = rows(ev, name)[:, 0]
        assert (got == np.float32(want)).all(), f"planted {mode}: {got.tolist()} for (thread, trip) {PLANTS}, expected {want}"
        worst = max(worst, w)
    return worst


# ---- k_distance_minmax: pair counts around the block size ----------------------------------------------------------------------------

EDGE_SHAPES = [(1, 1), (1, 255), (255, 1), (16, 16), (257, 1), (1, 257), (17, 31), (3000, 40)]


def minmax_pair_count_edges(lib, O, device=False):
    """random atoms in [-10, 50]: a fifth of them outside the 40 A cell; the same coordinates in an open cell"""
    worst = 0.0
    for na, nb in EDGE_SHAPES:
        rng = np.random.default_rng(1000 * na + nb)
        N = na + nb + 5
        coords = rng.uniform(-10.0, 50.0, (3, 3, N)).astype(np.float32)
        perm = rng.permutation(N).astype(np.int32)
        a, b = perm[:na], perm[na:na + nb]
        for box in (40.0, None):
            _, w = check(lib, O, coords, box, np.ones(N, np.float32), [("mn", a, b, L.DIST_MIN), ("mx", a, b, L.DIST_MAX)],
                         f"{na} x {nb} {'periodic' if box else 'open'}", device=device, ranges=[(0, 2), (2, 3)])
            worst = max(worst, w)
    return worst


# ---- ragged populations ---------------------------------------------------------------------------------------------------------------

RAGGED_P = 13


def _ragged_system(F, seed=13, box=40.0, to_cart=None):
    """P = 13 contexts, context i with 1 + (7 i mod 23) atoms in a and 1 + (11 i mod 37) in b (1 x 1 up to 22 x 30 and 2 x 37): compact
    clusters around random centres of the cell, some across its faces, drifting from frame to frame; shuffled atom order, masses
    between 1 and 40.  to_cart: a map of the coordinates (the triclinic case shears them)."""
    rng = np.random.default_rng(seed)
    na = [1 + (7 * i) % 23 for i in range(RAGGED_P)]
    nb = [1 + (11 * i) % 37 for i in range(RAGGED_P)]
    N = sum(na) + sum(nb) + 7
    perm = rng.permutation(N).astype(np.int32)
    a_sets, b_sets, k = [], [], 0
    for i in range(RAGGED_P):
        a_sets.append(perm[k:k + na[i]]); k += na[i]
        b_sets.append(perm[k:k + nb[i]]); k += nb[i]
    coords = rng.uniform(-10.0, box + 10.0, (F, 3, N))
    centre = rng.uniform(0.0, box, (RAGGED_P, 3))
    for f in range(F):
        for i in range(RAGGED_P):
            c = centre[i] + 0.4 * f
            coords[f][:, a_sets[i]] = c[:, None] + rng.normal(0.0, 2.0, (3, na[i]))
            coords[f][:, b_sets[i]] = c[:, None] + 5.0 + rng.normal(0.0, 2.5, (3, nb[i]))
    if to_cart is not None:
        coords = to_cart(coords)
    return coords.astype(np.float32), a_sets, b_sets, rng.uniform(1.0, 40.0, N).astype(np.float32)


def ragged_populations(lib, O, device=False):
    """F = 5 frames in one batch: B * P = 65 values, the first thread of a second block of k_distance_com"""
    coords, a_sets, b_sets, mass = _ragged_system(5)
    specs = [("c", a_sets, b_sets, L.DIST_COM, "pop"), ("mn", a_sets, b_sets, L.DIST_MIN, "pop"), ("mx", a_sets, b_sets, L.DIST_MAX, "pop")]
    worst = 0.0
    with _options(lib, batch_frames=0):
        for box in (40.0, None):
            ev, w = check(lib, O, coords, box, mass, specs, f"ragged {'periodic' if box else 'open'}", device=device)
            assert rows(ev, "c").shape == (5, RAGGED_P)
            worst = max(worst, w)
    # the masses matter: the restatement with unit weights gives other centres
    assert (R.com(coords, 40.0, a_sets, b_sets, mass) != R.com(coords, 40.0, a_sets, b_sets, None)).mean() > 0.5
    return worst


# ---- k_distance_com: thread slots and a long serial centre ----------------------------------------------------------------------------

def com_slots(lib, O, device=False):
    """P = 1: the last thread of the first block, a full block, the first thread of the second, a third block"""
    rng = np.random.default_rng(64)
    mass = rng.uniform(1.0, 40.0, 9).astype(np.float32)
    with _options(lib, batch_frames=0):
        for F in (63, 64, 65, 130):
            coords = rng.uniform(-5.0, 45.0, (F, 3, 9)).astype(np.float32)
            ev, _ = check(lib, O, coords, 40.0, mass, [("d", [4, 0, 7], [2, 8, 1, 5], L.DIST_COM)], f"com slots F={F}", device=device)
            assert rows(ev, "d").shape == (F, 1)


def com_large_set(lib, O, device=False):
    """5 000 atoms in a slab 14 A wide (less than half the 40 A cell) around the face x = 40, half of them stored wrapped to the far side
    of the cell, against one atom; with masses and with spec_dist_geometric_com"""
    rng = np.random.default_rng(5000)
    n, box, F = 5000, 40.0, 3
    coords = np.empty((F, 3, n + 1))
    coords[:, 0, :n] = rng.uniform(33.0, 47.0, (F, n))
    coords[:, 1:, :n] = rng.uniform(-6.0, 8.0, (F, 2, n))
    half = rng.random(n) < 0.5
    coords[:, :, :n][:, :, half] = np.mod(coords[:, :, :n][:, :, half], box)
    coords[:, :, n] = (20.0, 21.0, 19.0)
    coords = coords.astype(np.float32)
    mass = rng.uniform(1.0, 40.0, n + 1).astype(np.float32)
    a, b = rng.permutation(n).astype(np.int32), np.array([n], np.int32)
    got = {}
    for geometric in (0, 1):
        with _options(lib, spec_dist_geometric_com=geometric):
            ev, _ = check(lib, O, coords, box, mass, [("d", a, b, L.DIST_COM)], f"com of 5000 atoms geometric={geometric}", device=device,
                          geometric=bool(geometric), oracle_mass=np.ones_like(mass) if geometric else None)
        got[geometric] = rows(ev, "d")
    assert (got[0] != got[1]).all(), "the masses must move the centre"
    # the centre lies in the slab (x about 40, i.e. 0 after wrapping), 20 A from the atom along x: not at the far-side average
    assert (np.abs(got[1] - np.sqrt(20.0 ** 2 + 20.0 ** 2 + 18.0 ** 2)) < 1.0).all(), got[1].tolist()


# ---- k_distance_pair as a population --------------------------------------------------------------------------------------------------

PAIR_SHAPES = [(16, 16), (257, 1), (17, 16)]        # per = 256: one full block; 257: a second block of one thread; 272: gridDim.y = 2


def _pair_population(seed=5, to_cart=None, shapes=PAIR_SHAPES):
    rng = np.random.default_rng(seed)
    N, P, F = 400, 5, 3
    coords = rng.uniform(-10.0, 50.0, (F, 3, N))
    if to_cart is not None:
        coords = to_cart(coords)
    specs = []
    for na, nb in shapes:
        sets = [rng.permutation(N).astype(np.int32) for _ in range(P)]
        specs.append((f"p{na}x{nb}", [s[:na] for s in sets], [s[na:na + nb] for s in sets], L.DIST_PAIR, "pop"))
    return coords.astype(np.float32), specs


def pair_populations(lib, O, device=False):
    """every element of every row against the fp64 reference in row-major order (a outer, b inner, context by context)"""
    coords, specs = _pair_population()
    worst = 0.0
    for box in (40.0, None):
        ev, w = check(lib, O, coords, box, np.ones(coords.shape[2], np.float32), specs, f"pair population {'periodic' if box else 'open'}",
                      device=device)
        for sp in specs:
            assert rows(ev, sp[0]).shape == (3, 5 * len(sp[1][0]) * len(sp[2][0]))
        worst = max(worst, w)
    return worst


# ---- batching -------------------------------------------------------------------------------------------------------------------------

def batching(lib, O, device=False):
    """one script with all four kinds over 8 frames: whatever the batches, the rows are the same bits"""
    coords, a_sets, b_sets, mass = _ragged_system(8, seed=21)
    N = coords.shape[2]
    rng = np.random.default_rng(22)
    perm = rng.permutation(N).astype(np.int32)
    sets = [rng.permutation(N).astype(np.int32) for _ in range(5)]
    specs = [("c", perm[:6], perm[6:15], L.DIST_COM), ("mn", perm[:NA], perm[NA:NA + NB], L.DIST_MIN),
             ("mx", a_sets, b_sets, L.DIST_MAX, "pop"), ("p", [s[:17] for s in sets], [s[17:33] for s in sets], L.DIST_PAIR, "pop")]
    runs, worst = {}, 0.0
    for batch, dev in ((0, device), (1, device), (3, device), (0, False)):
        with _options(lib, batch_frames=batch):
            ev, w = check(lib, O, coords, 40.0, mass, specs, f"batch_frames={batch} {'device' if dev else 'host'} trajectory", device=dev)
        runs[(batch, dev)] = {sp[0]: rows(ev, sp[0]) for sp in specs}
        worst = max(worst, w)
    first = runs[(0, device)]
    for key, got in runs.items():
        for name, v in got.items():
            assert np.array_equal(v.view(np.int32), first[name].view(np.int32)), f"{name}: {key} differs from one batch"
    return worst


# ---- triclinic ------------------------------------------------------------------------------------------------------------------------

def _shear(coords, span=40.0):
    """coordinates generated for a cube of `span` -> the same fractions of the triclinic cell"""
    A = R.cell_matrix(TRICLINIC)
    return np.einsum("ij,fjn->fin", A, np.asarray(coords, np.float64) / span)


def triclinic(lib, O, device=False):
    rng = np.random.default_rng(77)
    F = 3
    # 300 x 41, overlapping sets: every b atom lies 1 to 3 A from some a atom, a spread over the cell and a fifth of a cell beyond
    frac = rng.uniform(-0.2, 1.2, (F, 3, NA + NB))
    coords = np.einsum("ij,fjn->fin", R.cell_matrix(TRICLINIC), frac)
    perm = rng.permutation(NA + NB).astype(np.int32)
    a, b = perm[:NA], perm[NA:]
    for f in range(F):
        off = rng.normal(size=(3, NB))
        off *= rng.uniform(1.0, 3.0, NB) / np.linalg.norm(off, axis=0)
        coords[f][:, b] = coords[f][:, rng.choice(a, NB, replace=False)] + off
    coords = coords.astype(np.float32)
    ev, _ = check(lib, O, coords, TRICLINIC, np.ones(NA + NB, np.float32), [("mn", a, b, L.DIST_MIN), ("mx", a, b, L.DIST_MAX)],
                  "triclinic 300 x 41", device=device)
    ref = R.min_images27(coords, TRICLINIC, a, b)
    quarter = R.cell_widths(TRICLINIC).min() / 4.0
    assert (ref < quarter).all(), f"the inputs must keep the minimum ({ref.tolist()}) below a quarter of the cell width ({quarter:.2f})"
    got = rows(ev, "mn")[:, 0].astype(np.float64)
    u = np.abs(got - ref) / (R.EPS * R.magnitude_tri(coords, TRICLINIC))
    print(f"triclinic 300 x 41 mn: max deviation {u.max():.2f} units of 2^-24 M from the 27-image fp64 search")
    assert (np.abs(got - ref) <= R.tolerance_tri(coords, TRICLINIC)).all(), f"{u.max():.2f} units from the 27-image search"
    # ragged COM population (restatement, bit for bit) and the 272-pair population (oracle)
    coords, a_sets, b_sets, mass = _ragged_system(5, seed=14, to_cart=_shear)
    check(lib, O, coords, TRICLINIC, mass, [("c", a_sets, b_sets, L.DIST_COM, "pop")], "triclinic ragged", device=device)
    coords, specs = _pair_population(seed=6, to_cart=_shear, shapes=[(17, 16)])
    check(lib, O, coords, TRICLINIC, np.ones(coords.shape[2], np.float32), specs, "triclinic pair population", device=device)
    return float(u.max())


# ---- script level ---------------------------------------------------------------------------------------------------------------------

SCRIPT = ('dm = distance_min(resname("ALA"), element(\'O\')); dx = distance_max(1:300, 301:341); '
          'dp = distance_min(1:2, element(\'O\')) in residue(2:5); dw = distance_min(resname("ALA"), element(\'O\') and water); '
          'dr = distance_max(1:2, element(\'O\') or element(\'H\')) in resname("ALA"); dc = distance(1:2, element(\'O\') or element(\'H\')) in resname("ALA");')


def script_level(lib, O, device=False):
    """residues of unequal size: the blob's last ALA has 5 atoms (N, C, C, O, C), so `in resname("ALA")` is a ragged population"""
    n_blob, n_atoms, box, F = 2005, 2005 + 3 * 120, 40.0, 3
    topo = synth.water_box_topology(n_atoms, n_blob=n_blob)
    coords = cases.host_frames(O, 9, n_atoms, box, F, n_blob=n_blob)
    ir_py, info = script.compile_script(SCRIPT, topo, lib=lib)
    ir_c = script.compile_script_native(SCRIPT, topo, lib=lib)
    assert ir_c.property_names() == ir_py.property_names() == ["dm", "dx", "dp", "dw", "dr", "dc"]
    assert ir_c.fingerprint() == ir_py.fingerprint(), "the two front-ends resolve the script to different sets"
    specs = []
    for name in ir_py.property_names():
        d = info[name]
        specs.append((name, d["a_sets"], d["b_sets"], KIND[d["kind"]], "pop") if "a_sets" in d else (name, d["a"], d["b"], KIND[d["kind"]]))
    assert info["dm"]["a"].size == 2005 and info["dm"]["b"].size == 201 + 120 and info["dw"]["b"].size == 120
    assert info["dx"]["a"].tolist() == list(range(300)) and info["dx"]["b"].tolist() == list(range(300, 341))
    assert [(x.tolist(), y.tolist()) for x, y in zip(info["dp"]["a_sets"], info["dp"]["b_sets"])] == \
        [([10 * r, 10 * r + 1], [10 * r + 3]) for r in range(1, 5)]
    assert [len(x) for x in info["dr"]["b_sets"]] == [5] * 200 + [1] and [len(x) for x in info["dc"]["b_sets"]] == [5] * 200 + [1]
    worst = 0.0
    for ir, what in ((ir_c, "native front-end"), (ir_py, "python front-end")):
        _, w = check(lib, O, coords, box, topo.mass, specs, f"script, {what}", device=device, ir=ir)
        worst = max(worst, w)
    return worst
