"""The SDF alignment stage (K3) held against tests/sdf_align_ref.py: k_sdf_ref_pose, k_sdf_align and k_sdf_group through direct calls of
vmd_hip_sdf_ref_pose / vmd_hip_sdf_align, run by tests/test_sdf_align_emu.py on the SIMT emulator and by tests/test_sdf_align_gpu.py on
the device.  The oracle repeats the kernel's operations in the kernel's order, so its bit-equality (cases.check_sdf) cannot see a mistake
made alike on both sides; the reference here is weighted Kabsch by SVD on structures whose whole form is known from their generation.

Per (frame b, structure k), `held` asserts
  well-conditioned (|N|_F / (l1 - l2) <= 1e3, asserted): |M64[:, :3] - R_ref|_max <= UNITS u + 4 * 2^-52, u = 2^-52 |N|_F / (l1 - l2);
  every pair: R orthonormal with determinant +1 within that bound (u of a degenerate pair taken as 2^-52), and the residual
      E(R) = sum w |R c - r|^2 <= E_opt + 2 UNITS 2^-52 |N|_F  (degenerate pairs - m <= 2, collinear, mirror images - are held by this alone);
  centre: c32 within 2^-24 |c| + cb of c_ref, cb = (m + 2) 2^-53 sum |w x| / sum w per axis, the bound of a sequential sum;
      M[:, 3] within |R| cb + 3 * 2^-53 |R| |c| of -R c_ref (the rounding of the stored product), and the centre recovered from it,
      c = -R^T M[:, 3], within cb + |R^T| (3 * 2^-53 |R| |c|) of c_ref (cb alone is missed by the recovered centre, emulator and
      device alike, by up to 2.96 x - structure_sizes m = 3 - on an axis whose coordinate is small beside the others: the stored
      product's rounding, not the sum; every case prints the figure);
  R32 == float32(M64[:, :3]) bit for bit; the sentinel tail behind B K entries of every output untouched.
Every case prints its worst deviation in units of u."""
import itertools
import math

import numpy as np

import cases
import distance_ref as D
import sdf_align_ref as R
from cell_build_cases import Buffers
from distance_cases import TRICLINIC, _options
import viamd_amd as V

TAIL = 16                                   # sentinel entries behind every output
ELEMENTS = np.float32([12.011, 14.007, 15.999, 1.008, 32.06])


def box9(x, y=None, z=None, tilt=(0.0, 0.0, 0.0)):
    e = np.float32([x, x if y is None else y, x if z is None else z])
    return np.concatenate([e, np.float32(1.0) / e, np.float32(tilt)]).astype(np.float32)


def rot(axis, deg):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    if deg == 0.0:
        return np.eye(3)
    if deg == 180.0:
        return 2.0 * np.outer(a, a) - np.eye(3)
    t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx


def random_rot(rng):
    return rot(rng.normal(size=3), rng.uniform(0.0, 180.0))


class Batch:
    """one launch: B frames, K structures of m atoms; the pose is structure 0 of frame 0"""

    def __init__(self, name, B, K, m, boxes, pbc, seed, extra=7, row_stride=None, frame_stride=None, mass="rows", trees=None,
                 kind="well", scatter=False):
        self.name, self.B, self.K, self.m, self.pbc = name, B, K, m, pbc
        self.rng = rng = np.random.default_rng(seed)
        self.N = N = K * m + extra
        self.rs = row_stride or N
        self.fs = frame_stride or 3 * self.rs
        assert self.rs >= N and self.fs >= 3 * self.rs
        self.boxes = np.ascontiguousarray(np.broadcast_to(boxes, (B, 9)), np.float32).copy()
        self.xyz = np.full(B * self.fs + TAIL, np.nan, np.float32)
        for b in range(B):                                       # every atom finite; the padding of rows and frames stays NaN
            for r in range(3):
                self.xyz[b * self.fs + r * self.rs: b * self.fs + r * self.rs + N] = rng.uniform(-50.0, 90.0, N).astype(np.float32)
        atoms = rng.permutation(N)[:K * m] if scatter else np.arange(K * m)
        self.structs = np.ascontiguousarray(atoms.reshape(K, m), np.int32)
        if isinstance(mass, str):
            base = rng.choice(ELEMENTS, m).astype(np.float32)
            mass = np.stack([base] * K) if mass == "same" else np.stack([rng.permutation(base) if k else base for k in range(K)])
        self.mass = None if mass is None else np.ascontiguousarray(mass, np.float32).reshape(K, m)
        self.order, self.parent = (None, None) if trees is None else (np.ascontiguousarray(t, np.int32).reshape(K, m) for t in trees)
        self.n = np.zeros((B, K, m, 3), np.int64)
        self.kind = np.full((B, K), kind, dtype=object)
        self._ref = None

    def A(self, b):
        return R.cell_matrix(self.boxes[b])

    def put(self, b, k, gen, extra_n=None):
        """store the whole structure gen float64 [m, 3]: every atom folded into the cell along the periodic axes (+ extra_n boxes)"""
        A, per = self.A(b), R.periodic_axes(self.pbc)
        s = np.linalg.solve(A, gen.T).T
        n = np.where(per[None, :], -np.floor(s), 0.0).astype(np.int64)
        if extra_n is not None:
            n = n + np.where(per[None, :], extra_n, 0)
        self.n[b, k] = n
        st = (gen + n.astype(float) @ A.T).astype(np.float32)
        for r in range(3):
            self.xyz[b * self.fs + r * self.rs + self.structs[k]] = st[:, r]

    def stored(self, b, k):
        return np.stack([self.xyz[b * self.fs + r * self.rs + self.structs[k]] for r in range(3)], axis=1)

    def weights(self, k):
        return np.ones(self.m) if self.mass is None else self.mass[k].astype(np.float64)

    def root(self, k):
        return 0 if self.order is None else int(self.order[k, 0])

    def parents(self, k):
        return R.chain_parent(self.m) if self.parent is None else self.parent[k]

    def whole(self, b, k):
        x = R.whole(self.stored(b, k), self.n[b, k], self.A(b), self.root(k))
        frac = R.bond_fractions(x, self.parents(k), self.A(b), self.pbc)
        assert frac < 0.45, f"{self.name}: a bond of ({b}, {k}) spans {frac:.3f} of the cell"
        return x

    def reference(self):
        """-> (pose, pose centre, pose mag, fits [B][K]), once"""
        if self._ref is None:
            pose, pc, pmag = R.pose_of(self.weights(0), self.whole(0, 0))
            fits = [[R.fit(self.weights(k), self.whole(b, k), pose) for k in range(self.K)] for b in range(self.B)]
            self._ref = pose, pc, pmag, fits
        return self._ref


class Out:
    pass


def launch(lib, bt, gpu, group=True, mass="own"):
    """vmd_hip_sdf_ref_pose on frame 0, then vmd_hip_sdf_align on the batch -> Out with the fetched arrays"""
    B, K, m = bt.B, bt.K, bt.m
    BK = B * K
    nan32, nan64 = (lambda n: np.full(n, np.nan, np.float32)), (lambda n: np.full(n, np.nan, np.float64))
    ms = bt.mass if isinstance(mass, str) else mass
    buf = Buffers(gpu, xyz=bt.xyz, boxes=bt.boxes.reshape(-1), structs=bt.structs.reshape(-1), mass=None if ms is None else ms.reshape(-1),
                  pose=nan64(3 * m + TAIL), R32=nan32(9 * BK + TAIL), c32=nan32(3 * BK + TAIL), M64=nan64(12 * BK + TAIL),
                  group=nan32(4 * B + TAIL) if group else None,
                  order=None if bt.order is None else bt.order.reshape(-1), parent=None if bt.parent is None else bt.parent.reshape(-1),
                  tree_pos=None if bt.order is None else nan64(3 * m * BK + TAIL))
    assert lib.vmd_hip_sdf_ref_pose(None, buf["xyz"], bt.rs, buf["boxes"], bt.pbc, buf["structs"], buf["mass"], m, buf["pose"],
                                    buf["order"], buf["parent"]) == 0
    assert lib.vmd_hip_sdf_align(None, buf["xyz"], bt.fs, bt.rs, buf["boxes"], bt.pbc, B, buf["structs"], buf["mass"], K, m, buf["pose"],
                                 buf["R32"], buf["c32"], buf["M64"], buf["group"], buf["order"], buf["parent"], buf["tree_pos"]) == 0
    o = Out()
    o.raw = {k: buf.fetch(k).copy() for k in ("pose", "R32", "c32", "M64") + (("group",) if group else ()) + (("tree_pos",) if bt.order is not None else ())}
    for k, n in (("pose", 3 * m), ("R32", 9 * BK), ("c32", 3 * BK), ("M64", 12 * BK), ("group", 4 * B), ("tree_pos", 3 * m * BK)):
        if k in o.raw:
            assert np.isnan(o.raw[k][n:]).all() and o.raw[k][n:].size == TAIL, f"{bt.name}: the tail behind {k} was written"
            assert np.isfinite(o.raw[k][:n]).all(), f"{bt.name}: {k} holds entries that were not written"
    o.pose = o.raw["pose"][:3 * m].reshape(m, 3)
    o.R32 = o.raw["R32"][:9 * BK].reshape(B, K, 3, 3)
    o.c32 = o.raw["c32"][:3 * BK].reshape(B, K, 3)
    o.M64 = o.raw["M64"][:12 * BK].reshape(B, K, 3, 4)
    o.group = o.raw["group"][:4 * B].reshape(B, 4) if group else None
    return o


def held(bt, o):
    """the assertions of the module's head; -> worst deviation of a compared matrix in u"""
    pose, _, _, fits = bt.reference()
    worst = worst_c = worst_bare = worst_e = 0.0
    worst_c32 = -math.inf
    for b, k in itertools.product(range(bt.B), range(bt.K)):
        f, M, what = fits[b][k], o.M64[b, k], f"{bt.name} ({b}, {k})"
        Rk, t = M[:, :3], M[:, 3]
        w = bt.weights(k)
        well = bt.kind[b, k] == "well"
        if well:
            assert f.cond <= R.COND_MAX, f"{what}: conditioning {f.cond:.3g} of a case that compares the matrix"
            tol = R.UNITS * f.u + 4.0 * R.EPS
            dev = float(np.abs(Rk - f.R).max())
            worst = max(worst, dev / f.u)
            assert dev <= tol, f"{what}: rotation {dev / f.u:.2f} u from the reference (bound {R.UNITS} u + 4 * 2^-52)"
        else:
            tol = R.UNITS * R.EPS + 4.0 * R.EPS
        assert np.abs(Rk @ Rk.T - np.eye(3)).max() <= tol, f"{what}: R is not orthonormal"
        assert abs(np.linalg.det(Rk) - 1.0) <= tol, f"{what}: det R = {np.linalg.det(Rk)}"
        # The fp64 centre exists only inside M[:, 3] = fl(-(R c)): three products and two sums, each rounded, so what comes back out
        # of it carries up to 3 * 2^-53 |R| |c| of every axis on every other - more than the sum's own bound on an axis whose
        # coordinate is small beside the others.  The recovery itself adds nothing: extended precision, one step of refinement
        # against R not being orthonormal to the last bit.
        Rl, tl = Rk.astype(np.longdouble), t.astype(np.longdouble)
        cl = -(Rl.T @ tl)
        c = (cl - Rl.T @ (tl + Rl @ cl)).astype(np.float64)
        cb = R.centre_bound(bt.m, f.mag)
        stored = 3.0 * 2.0 ** -53 * (np.abs(Rk) @ np.abs(f.c))              # the rounding of M[:, 3] as the kernel stores it
        cr = cb + np.abs(Rk).T @ stored
        worst_c = max(worst_c, float((np.abs(c - f.c) / np.where(cr > 0, cr, 1.0)).max()))
        worst_bare = max(worst_bare, float((np.abs(c - f.c) / np.where(cb > 0, cb, 1.0)).max()))
        assert (np.abs(c - f.c) <= cr).all(), f"{what}: centre off by {np.abs(c - f.c)} (bound {cr})"
        c32 = o.c32[b, k].astype(np.float64)
        worst_c32 = max(worst_c32, float(((np.abs(c32 - f.c) - 2.0 ** -24 * np.abs(f.c)) / np.where(cb > 0, cb, 1.0)).max()))
        assert (np.abs(c32 - f.c) <= cb + 2.0 ** -24 * np.abs(f.c)).all(), f"{what}: c32 off by {np.abs(c32 - f.c)}"
        assert (np.abs(t + Rk @ f.c) <= np.abs(Rk) @ cb + stored).all(), f"{what}: M[:, 3] is not -R c: {t + Rk @ f.c}"
        # the residual of the kernel's own rotation about the reference's centre
        e = R.residual(w, Rk, f.c, f.x, pose)
        slack = 2.0 * R.UNITS * R.EPS * f.normN
        worst_e = max(worst_e, (e - f.e_opt) / slack if slack > 0 else 0.0)
        assert e <= f.e_opt + slack, f"{what}: residual {e} above the optimum {f.e_opt} by more than {slack}"
        np.testing.assert_array_equal(o.R32[b, k].view(np.uint32), Rk.astype(np.float32).view(np.uint32), err_msg=f"{what}: R32 is not float32(M64)")
    print(f"sdf_align {bt.name}: B = {bt.B}, K = {bt.K}, m = {bt.m}: worst rotation {worst:.2f} u (bound {R.UNITS:.0f}), worst centre "
          f"{worst_c:.2f} of its bound ({worst_bare:.2f} of the sum's bound alone, c32 {max(worst_c32, 0.0):.2f}), worst residual excess {worst_e:.3f} of its bound")
    return worst


def run(lib, bt, gpu, **kw):
    o = launch(lib, bt, gpu, **kw)
    held(bt, o)
    return o


# ---- thread_slots ---------------------------------------------------------------------------------------------------------------------

SLOTS = [(1, 1), (63, 1), (64, 1), (65, 1), (13, 5), (10, 13), (1, 70)]
ANGLES = (0.0, 180.0, 179.9)


def slots_batch(B, K):
    bt = Batch(f"thread_slots {B} x {K}", B, K, 9, box9(40.0), 7, seed=100 * B + K, mass="same")
    rng = bt.rng
    template = rng.normal(0.0, 1.6, (9, 3))
    for i, (b, k) in enumerate(itertools.product(range(B), range(K))):
        Rm = rot(rng.normal(size=3), ANGLES[i % 7] if i % 7 < 3 else rng.uniform(0.0, 180.0))
        bt.put(b, k, template @ Rm.T + rng.uniform(0.0, 40.0, 3) + rng.normal(0.0, 0.05, (9, 3)))
    return bt


def slots_batches():
    return [slots_batch(B, K) for B, K in SLOTS]


def thread_slots(lib, device=False):
    for bt in slots_batches():
        run(lib, bt, device)


# ---- structure_sizes ------------------------------------------------------------------------------------------------------------------

def size_batch(m, what):
    B, K = 3, 2
    box = 90.0 if m >= 64 else 40.0
    bt = Batch(f"structure_sizes m = {m} {what}", B, K, m, box9(box), 7, seed=7 * m + len(what), mass="same",
               kind="well" if what in ("", "planar") else "degenerate")
    rng = bt.rng
    if what == "collinear":
        template = np.outer(np.cumsum(rng.uniform(1.0, 2.0, m)), rng.normal(size=3))
    elif what == "planar":
        template = np.concatenate([rng.normal(0.0, 1.6, (m, 2)), np.zeros((m, 1))], axis=1)
    elif what == "mirror":                                       # a tetrahedron of definite handedness
        template = np.array([[2.0, 0.0, 0.0], [0.0, 1.5, 0.0], [0.0, 0.0, 1.0], [-1.0, -1.0, -1.0]]) + rng.normal(0.0, 0.1, (4, 3))
    else:
        template = rng.normal(0.0, 1.6 if m < 64 else 4.0, (m, 3))
    for b, k in itertools.product(range(B), range(K)):
        t = template * np.array([-1.0, 1.0, 1.0]) if what == "mirror" and (b, k) != (0, 0) else template
        bt.put(b, k, t @ random_rot(rng).T + rng.uniform(0.0, box, 3) + rng.normal(0.0, 0.05 if m > 2 else 0.0, (m, 3)))
    return bt


SIZES = [(1, "single"), (2, "pair"), (5, "collinear"), (3, "planar"), (4, "mirror"), (64, ""), (65, ""), (1000, "")]


def size_batches():
    return [size_batch(m, what) for m, what in SIZES]


def structure_sizes(lib, device=False):
    for bt in size_batches():
        o = run(lib, bt, device)
        if bt.m == 1:
            for b, k in itertools.product(range(bt.B), range(bt.K)):
                np.testing.assert_array_equal(o.M64[b, k, :, :3], np.eye(3), err_msg="m = 1: R is the identity, exactly")
                np.testing.assert_array_equal(o.c32[b, k].view(np.uint32), bt.stored(b, k)[0].view(np.uint32), err_msg="m = 1: c32 is the atom")
        if "mirror" in bt.name:
            _, _, _, fits = bt.reference()
            assert all(np.linalg.det(fits[b][k].S) < 0 for b in (1, 2) for k in (0, 1)), "the mirror images need the determinant correction"


# ---- masses ---------------------------------------------------------------------------------------------------------------------------

def mass_batch(name, rows, seed, K=3, m=9):
    B = 3
    bt = Batch(f"masses {name}", B, K, m, box9(40.0), 7, seed=seed, mass=rows)
    rng = bt.rng
    template = rng.normal(0.0, 1.6, (m, 3))
    for b, k in itertools.product(range(B), range(K)):
        bt.put(b, k, template @ random_rot(rng).T + rng.uniform(0.0, 40.0, 3) + rng.normal(0.0, 0.05, (m, 3)))
    return bt


def mass_batches():
    rng = np.random.default_rng(77)
    rows = rng.uniform(1.0, 40.0, (3, 9)).astype(np.float32)                     # a different row per structure
    heavy = np.where(rng.permutation(9)[None, :] < 3, np.float32(197.0), np.float32(1.0)) * np.ones((3, 1), np.float32)
    heavy[1], heavy[2] = np.roll(heavy[0], 2), np.roll(heavy[0], 5)
    virtual = rows.copy()
    virtual[0, 3] = virtual[1, 0] = virtual[2, 8] = 0.0                          # one massless site per structure
    return [mass_batch("none", None, 70), mass_batch("rows", rows, 71), mass_batch("1 : 197", heavy, 72), mass_batch("virtual site", virtual, 73)]


def masses(lib, device=False):
    for bt in mass_batches():
        o = run(lib, bt, device)
        if bt.mass is None:
            ones = launch(lib, bt, device, mass=np.ones((bt.K, bt.m), np.float32))
            for k in o.raw:
                np.testing.assert_array_equal(o.raw[k].view(np.uint8), ones.raw[k].view(np.uint8), err_msg=f"mass == NULL against ones: {k}")
        if "rows" in bt.name:
            # the [K][m] indexing: with structure 0's row for every structure the centres move by far more than any bound
            _, _, _, fits = bt.reference()
            wrong = R.centre(bt.weights(0), fits[1][2].x)[0]
            assert np.abs(wrong - fits[1][2].c).max() > 1.0e-2


# ---- unwrap_chain ---------------------------------------------------------------------------------------------------------------------

def chain_batch(name, box, seed):
    B, K, m = 2, 5, 9
    bt = Batch(f"unwrap_chain {name}", B, K, m, box, 7, seed=seed)
    rng = bt.rng
    Lx, Ly, Lz = (float(v) for v in box[:3])
    template = rng.normal(0.0, 1.6, (m, 3))
    spots = [(0.2, Ly / 2, Lz / 2), (0.2, Ly - 0.1, Lz / 2), (0.1, 0.1, Lz - 0.1), (Lx / 2, Ly / 2, 0.0)]      # face, edge, corner, face
    far = np.zeros((m, 3), np.int64)
    far[1::2] = (3, -3, 0)                                                      # every other atom three boxes away from its neighbour
    far[4] = (-3, 0, 3)
    for b in range(B):
        for k in range(4):
            gen = template @ random_rot(rng).T + np.array(spots[k]) + rng.normal(0.0, 0.05, (m, 3))
            bt.put(b, k, gen, extra_n=far if k == 3 else None)
            assert k == 3 or np.abs(bt.n[b, k] - bt.n[b, k][0]).any(), "the structure does not cross the cell's boundary"
        bt.put(b, 4, template @ random_rot(rng).T + rng.uniform(0.0, Lx, 3))
    return bt


def walk_batch():
    """a 60 atom random walk of 1.5 A bonds with a drift: its contour, 88.5 A, is longer than four 20 A boxes"""
    B, K, m = 2, 2, 60
    bt = Batch("unwrap_chain walk", B, K, m, box9(20.0), 7, seed=61)
    rng = bt.rng
    steps = rng.normal(size=(m, 3)) + np.array([1.2, 0.8, 0.0])
    steps = 1.5 * steps / np.linalg.norm(steps, axis=1)[:, None]
    template = np.cumsum(steps, axis=0)
    assert np.ptp(template, axis=0).max() > 40.0
    for b, k in itertools.product(range(B), range(K)):
        bt.put(b, k, template @ random_rot(rng).T + rng.uniform(0.0, 20.0, 3) + rng.normal(0.0, 0.05, (m, 3)))
    return bt


def chain_batches():
    return [chain_batch("cube 20", box9(20.0), 60), chain_batch("50 x 40 x 30", box9(50.0, 40.0, 30.0), 62), walk_batch()]


def unwrap_chain(lib, device=False):
    for bt in chain_batches():
        run(lib, bt, device)


# ---- unwrap_tree ----------------------------------------------------------------------------------------------------------------------

def chain_made(stored, A, per):
    """what a walk along the index order makes of the stored atoms (fp64; only to show that it is NOT the structure)"""
    x = stored.astype(np.float64).copy()
    Ai = np.linalg.inv(A)
    for a in range(1, len(x)):
        s = Ai @ (x[a] - x[a - 1])
        x[a] = x[a - 1] + A @ np.where(per, s - np.rint(s), s)
    return x


def tree_batch():
    """B K = 65 structures of 9 atoms in a 20 A cube, a different spanning tree per structure.  Every tree edge is short (6.5 A or less
    per axis); along x some index neighbours are 12 A or more apart - over half the cell - so a walk along the index order folds them
    onto the wrong image.  The planted rotations turn about x, which keeps that so in every frame."""
    B, K, m, box = 13, 5, 9, 20.0
    rng = np.random.default_rng(91)
    order, parent, templates = [], [], []
    for k in range(K):
        while True:
            if k == 0:                                           # a star about atom 4
                o = np.array([4, 8, 0, 6, 2, 7, 1, 5, 3])
                p = np.where(np.arange(m) == 4, -1, 4)
            elif k == 1:                                         # the chain, walked from its last atom
                o = np.arange(m)[::-1].copy()
                p = np.where(np.arange(m) == m - 1, -1, np.arange(m) + 1)
            else:                                                # a random tree: a child is visited before atoms of lower index
                o = rng.permutation(m)
                p = np.full(m, -1)
                for t in range(1, m):
                    p[o[t]] = o[rng.integers(max(0, t - 3), t)]
            x = np.zeros((m, 3))
            for t in range(1, m):                                # the star's arms alternate between +x and -x by index
                sx = (1.0 if o[t] % 2 else -1.0) if k == 0 else 1.0
                x[o[t]] = x[p[o[t]]] + np.array([6.0 * sx, rng.uniform(-3.0, 3.0), rng.uniform(-3.0, 3.0)])
            if k < 2 or (o[0] != 0 and any(o[t] > o[t + 1] for t in range(1, m - 1)) and np.abs(np.diff(x[:, 0])).max() >= 12.0):
                break
        assert np.abs(np.diff(x[:, 0])).max() >= 12.0 or k == 1
        order.append(o); parent.append(p); templates.append(x)
    bt = Batch("unwrap_tree", B, K, m, box9(box), 7, seed=92, trees=(np.stack(order), np.stack(parent)))
    for b, k in itertools.product(range(B), range(K)):
        Rm = rot([1.0, 0.0, 0.0], bt.rng.uniform(0.0, 360.0))
        bt.put(b, k, templates[k] @ Rm.T + bt.rng.uniform(0.0, box, 3) + bt.rng.normal(0.0, 0.05, (m, 3)))
    return bt


def unwrap_tree(lib, device=False):
    bt = tree_batch()
    assert bt.B * bt.K == 65
    per = R.periodic_axes(bt.pbc)
    for b, k in itertools.product(range(bt.B), range(bt.K)):
        off = np.abs(chain_made(bt.stored(b, k), bt.A(b), per) - R.whole(bt.stored(b, k), bt.n[b, k], bt.A(b), bt.root(k))).max()
        assert off > 1.0, f"unwrap_tree ({b}, {k}): the index chain would make this structure whole as well ({off:.3f} A)"
    run(lib, bt, device)


# ---- cells ----------------------------------------------------------------------------------------------------------------------------

def cell_batch(name, boxes, pbc, seed, B=3):
    K, m = 3, 9
    bt = Batch(f"cells {name}", B, K, m, boxes, pbc, seed=seed)
    rng = bt.rng
    per = R.periodic_axes(pbc)
    # a rod: hops of 12 A - more than half the nominal 20 A edge - along every open axis, short ones along the periodic axes
    hop = np.where(per, 1.0, 12.0)
    template = np.cumsum(rng.uniform(0.85, 1.0, (m, 3)) * hop * rng.choice([-1.0, 1.0], (m, 3)), axis=0) if not per.all() else rng.normal(0.0, 1.6, (m, 3))
    assert per.all() or np.abs(np.diff(template, axis=0))[:, ~per].min() > 10.0
    # rotations that keep the long hops on the open axes: any (all periodic or all open), else about the axis that differs from the other two
    odd = int(np.argmax(per)) if per.sum() == 1 else int(np.argmin(per))
    far = np.zeros((m, 3), np.int64)
    far[2::3] = (2, -1, 1)
    for b, k in itertools.product(range(B), range(K)):
        Rm = random_rot(rng) if per.all() or not per.any() else rot(np.eye(3)[odd], rng.uniform(0.0, 180.0))
        e = bt.boxes[b, :3].astype(float)
        bt.put(b, k, template @ Rm.T + rng.uniform(0.0, 1.0, 3) * e + rng.normal(0.0, 0.05, (m, 3)), extra_n=far if k == 1 else None)
    return bt


def cell_batches():
    out = [cell_batch("triclinic", box9(*TRICLINIC[:3], tilt=TRICLINIC[3:]), 15, 80)]
    out += [cell_batch(f"pbc {f}", box9(20.0), f, 81 + f) for f in (0, 1, 3, 5, 6)]
    out.append(cell_batch("a box per frame", np.stack([box9(20.0 + 1.5 * b, 22.0 - b, 19.0 + 0.5 * b * b) for b in range(4)]), 7, 90, B=4))
    out.append(cell_batch("a triclinic box per frame", np.stack([box9(40.0 + b, 42.0, 44.0 - b, tilt=(5.0 + b, -3.0, 4.0 - b)) for b in range(3)]), 15, 91))
    return out


def cells(lib, device=False):
    for bt in cell_batches():
        run(lib, bt, device)


# ---- strides --------------------------------------------------------------------------------------------------------------------------

def stride_batch():
    B, K, m, extra = 3, 4, 9, 40
    N = K * m + extra
    bt = Batch("strides", B, K, m, box9(40.0), 7, seed=95, extra=extra, row_stride=N + 5, frame_stride=3 * (N + 5) + 11, scatter=True)
    rng = bt.rng
    template = rng.normal(0.0, 1.6, (m, 3))
    for b, k in itertools.product(range(B), range(K)):
        bt.put(b, k, template @ random_rot(rng).T + rng.uniform(0.0, 40.0, 3) + rng.normal(0.0, 0.05, (m, 3)))
    assert np.isnan(bt.xyz).sum() == B * (3 * 5 + 11) + TAIL and (np.diff(bt.structs.reshape(-1)) < 0).any()
    return bt


def strides(lib, device=False):
    run(lib, stride_batch(), device)


# ---- ref_pose -------------------------------------------------------------------------------------------------------------------------

def ref_pose(lib, device=False):
    tb = tree_batch()
    flat = Batch("ref_pose tree, no masses", tb.B, tb.K, tb.m, tb.boxes, tb.pbc, seed=1, mass=None, trees=(tb.order, tb.parent))
    flat.xyz, flat.n = tb.xyz, tb.n
    for bt in (chain_batches()[0], walk_batch(), mass_batches()[0], mass_batches()[3], tb, flat):
        o = launch(lib, bt, device)
        pose, c, mag, _ = bt.reference()
        x = pose + c
        w = bt.weights(0)
        cb = R.centre_bound(bt.m, mag)
        tol = cb[None, :] + R.EPS * np.abs(x)
        dev = np.abs(o.pose - pose)
        assert (dev <= tol).all(), f"ref_pose {bt.name}: the pose is off by {dev.max()} (bound {tol.max()})"
        s = np.array([math.fsum(w * o.pose[:, a]) for a in range(3)]) / math.fsum(w)
        assert (np.abs(s) <= cb + R.EPS * np.abs(x).max(0)).all(), f"ref_pose {bt.name}: the pose's weighted sum is {s}"
        print(f"sdf_align ref_pose {bt.name}: worst deviation {(dev / tol).max():.3f} of its bound, weighted sum {np.abs(s).max():.2e}")


# ---- group ----------------------------------------------------------------------------------------------------------------------------

def group_batch(B, K, boxes, pbc, seed, name):
    m = 5
    bt = Batch(f"group {name} B = {B}, K = {K}", B, K, m, boxes, pbc, seed=seed)
    rng = bt.rng
    template = rng.normal(0.0, 1.2, (m, 3))
    for b in range(B):
        e = bt.boxes[b, :3].astype(float)
        hub = np.array([0.5 if b % 2 else e[0] - 0.5, rng.uniform(0.0, e[1]), 0.3 if b % 3 == 0 else rng.uniform(0.0, e[2])])
        for k in range(K):                                       # the centres lie on both sides of the x = 0 face
            off = rng.normal(size=3) * np.array([3.0, 2.0, 2.0]) * (0.0 if k == 0 else 1.0)
            bt.put(b, k, template @ random_rot(rng).T + hub + off + rng.normal(0.0, 0.05, (m, 3)))
    return bt


def group(lib, device=False):
    tri = box9(*TRICLINIC[:3], tilt=TRICLINIC[3:])
    for bt in [group_batch(B, 4, box9(30.0, 26.0, 22.0), 7, 50 + B, "orthorhombic") for B in (1, 64, 65)] + \
              [group_batch(65, 1, box9(30.0), 7, 49, "one structure"), group_batch(65, 4, tri, 15, 48, "triclinic"),
               group_batch(3, 6, box9(30.0), 5, 47, "pbc 5")]:
        o = launch(lib, bt, device)
        per = R.periodic_axes(bt.pbc)
        worst = 0.0
        for b in range(bt.B):
            g, c = o.group[b], o.c32[b].astype(np.float64)
            np.testing.assert_array_equal(g[:3].view(np.uint32), o.c32[b, 0].view(np.uint32), err_msg=f"{bt.name}: frame {b}: g[0:3] is not c32[b][0]")
            if bt.K == 1:
                assert g[3] == np.float32(0.01), f"{bt.name}: frame {b}: radius {g[3]} of a single structure"
                continue
            d = max(R.min_image27(c[k] - c[0], bt.A(b), per) for k in range(1, bt.K))
            assert float(g[3]) >= d, f"{bt.name}: frame {b}: radius {g[3]} below the farthest centre at {d}: the scatter would drop hits"
            worst = max(worst, float(g[3]) - d)
            if not bt.pbc & 8:
                up = 1.0005 * d + 0.01 + D.UNITS * D.EPS * max(float(bt.boxes[b, :3].max()), float(np.abs(c).max()))
                assert float(g[3]) <= up, f"{bt.name}: frame {b}: radius {g[3]} above {up}"
        print(f"sdf_align {bt.name}: largest margin of the radius {worst:.4f} A")
        if bt.B == 65 and bt.K == 4 and not bt.pbc & 8:
            assert any(abs(o.c32[b, k, 0] - o.c32[b, 0, 0]) > 15.0 for b in range(bt.B) for k in range(bt.K)), "no pair of centres across the face"
            bare = launch(lib, bt, device, group=False)              # group == NULL: accepted, the other outputs as before
            for k in bare.raw:
                np.testing.assert_array_equal(bare.raw[k].view(np.uint8), o.raw[k].view(np.uint8), err_msg=f"group == NULL changes {k}")


# ---- evaluator_level ------------------------------------------------------------------------------------------------------------------

def evaluator_matrices(lib, device=False):
    """ScriptIR.add_sdf, frame_range under batch_frames 0, 1 and 3, ScriptEval.sdf_matrices of every frame; bonds handed over: the rings of
    cases.bonded_ring_case, which only the bond tree makes whole (breadth first from local atom 0, so the root is atom 0)"""
    coords, structures, mass, bonds, tgt, gen = cases.bonded_ring_case(None, frames=5)
    F, _, N = coords.shape
    K, m = structures.shape
    box = 24.0
    vcell = V.make_unitcell(box)
    A = R.cell_matrix(box9(box))
    stored = np.moveaxis(coords[:, :, :K * m].reshape(F, 3, K, m), 1, 3).astype(np.float64)
    n = np.rint((stored - gen) / box).astype(np.int64)                   # the lattice vector np.mod added to every atom
    assert np.abs(stored - (gen + n * box)).max() < 1.0e-5 and n.any()
    x = [[R.whole(coords[f][:, structures[k]].T, n[f, k], A, 0) for k in range(K)] for f in range(F)]
    ring = {(int(a), int(b)) for a, b in bonds} | {(int(b), int(a)) for a, b in bonds}
    for f, k in itertools.product(range(F), range(K)):                     # every bond is a short hop, whatever tree the library builds from them
        par = [-1] + [next(c for c in range(m) if (int(structures[k, a]), int(structures[k, c])) in ring) for a in range(1, m)]
        assert R.bond_fractions(x[f][k], par, A, 7) < 0.45
    pose, _, _ = R.pose_of(mass[structures[0]], x[0][0])
    fits = [[R.fit(mass[structures[k]], x[f][k], pose) for k in range(K)] for f in range(F)]
    volumes = []
    worst = 0.0
    for bf in (0, 1, 3):
        with _options(lib, batch_frames=bf):
            ir = V.ScriptIR(lib)
            ir.add_sdf("v", structures, tgt, 9.0)
            ev = V.ScriptEval(F, ir)
            sysm = V.MolSystem(N, mass=mass, unitcell=vcell, bonds=bonds)
            traj = cases.make_traj(lib, coords, vcell, device)
            assert ev.frame_range(sysm, traj, 0, F)
            volumes.append(ev.property_data("v").counts.copy())
            for f in range(F):
                M4, ext = ev.sdf_matrices("v", sysm, traj, f)
                assert ext == 9.0 and M4.shape == (K, 4, 4)
                for k in range(K):
                    ft = fits[f][k]
                    assert ft.cond <= R.COND_MAX
                    rb = R.UNITS * ft.u + 4.0 * R.EPS
                    dev = np.abs(M4[k, :3, :3].astype(np.float64) - ft.R)
                    assert (dev <= rb + 2.0 ** -24 * np.abs(ft.R)).all(), f"batch_frames {bf}, frame {f}, structure {k}: rotation off by {dev.max()}"
                    t = -(ft.R @ ft.c)
                    tb = 2.0 ** -24 * np.abs(t) + rb * np.abs(ft.c).sum() + np.abs(ft.R) @ R.centre_bound(m, ft.mag) + 4.0 * 2.0 ** -53 * (np.abs(ft.R) @ np.abs(ft.c))
                    assert (np.abs(M4[k, :3, 3].astype(np.float64) - t) <= tb).all(), f"batch_frames {bf}, frame {f}, structure {k}: translation"
                    np.testing.assert_array_equal(M4[k, 3], np.float32([0, 0, 0, 1]))
                    worst = max(worst, float((dev / (rb + 2.0 ** -24 * np.abs(ft.R))).max()))
    assert volumes[0].sum() > 0
    for v in volumes[1:]:
        np.testing.assert_array_equal(v, volumes[0], err_msg="the volume depends on batch_frames")
    print(f"sdf_align evaluator_level: matrices of {F} frames x {K} structures, worst {worst:.3f} of the fp32 bound")


def wide_group(lib, O, device=False):
    """K = 5 structures spread over a periodic 30 A cube: the group radius exceeds half the edge, and every voxel still equals the
    oracle's, whose scatter tests every (atom, structure) pair without a pre-filter"""
    box, K, m = 30.0, 5, 6
    coords, structures, mass = cases.sdf_system(O, 31, 1500, box, 3, K=K, m=m)
    spots = np.array([[2.0, 2.0, 2.0], [17.0, 3.0, 16.0], [3.0, 17.0, 18.0], [16.0, 16.0, 3.0], [15.0, 15.0, 15.0]])
    rng = np.random.default_rng(32)
    template = rng.normal(0.0, 1.3, (m, 3))
    for f in range(coords.shape[0]):
        for k in range(K):
            coords[f, :, k * m:(k + 1) * m] = np.mod(template @ random_rot(rng).T + spots[k] + rng.normal(0.0, 0.3, 3), box).T.astype(np.float32)
    d = spots[1:] - spots[0]
    d -= box * np.rint(d / box)
    assert np.sqrt((d * d).sum(1)).max() - 1.0 > 0.5 * box, "the group radius does not exceed half the edge"
    tgt = np.arange(K * m, coords.shape[2], dtype=np.int32)
    cases.check_sdf(lib, O, coords, box, structures, mass, tgt, 6.0, device=device)


def w_min(box6):
    """the smallest cell width as vmd_sdf_near computes it, float32"""
    f = np.float32
    Lx, Ly, Lz, xy, xz, yz = (f(v) for v in box6)
    iLy, iLz = f(1.0) / Ly, f(1.0) / Lz
    ty, tx1, tx2 = yz * iLz, xy * iLy, (xy * yz - Ly * xz) * (iLy * iLz)
    wy = Ly / np.sqrt(f(1.0) + ty * ty, dtype=f)
    wx = Lx / np.sqrt(f(1.0) + tx1 * tx1 + tx2 * tx2, dtype=f)
    return min(Lz, wx, wy)


def triclinic_reach(lib, O, device=False):
    """the triclinic cell with the filter's reach just below and just above 0.499 w_min: on one side the one-sphere test is used, on the
    other every atom goes to the K tests; both sides equal the oracle voxel for voxel"""
    K, m, F = 3, 6, 3
    box = TRICLINIC
    coords, structures, mass = cases.sdf_system(O, 33, 1500, box[0], F, K=K, m=m)
    rng = np.random.default_rng(34)
    template = rng.normal(0.0, 1.3, (m, 3))
    A = D.cell_matrix(box)
    cell_of = lambda p: (A @ (np.linalg.solve(A, p.T) % 1.0)).T
    com = np.zeros((F, K, 3))
    for f in range(F):
        hub = np.array([1.0, 25.0, 1.0]) + rng.normal(0.0, 0.5, 3)
        for k in range(K):
            pts = template @ random_rot(rng).T + hub + (rng.normal(0.0, 1.5, 3) if k else 0.0)
            com[f, k] = (mass[structures[k]].astype(np.float64)[:, None] * pts).sum(0) / mass[structures[k]].astype(np.float64).sum()
            coords[f, :, k * m:(k + 1) * m] = cell_of(pts).T.astype(np.float32)
    coords[:, :, K * m:] = np.moveaxis(np.stack([cell_of(rng.uniform(0.0, 1.0, (coords.shape[2] - K * m, 3)) @ A.T) for _ in range(F)]), 1, 2)
    # the group radius of frame f, as k_sdf_group forms it from the centres of mass (all of them a few A apart: no image is involved)
    radius = np.array([1.0005 * max(np.linalg.norm(com[f, k] - com[f, 0]) for k in range(1, K)) + 0.01 for f in range(F)])
    limit = 0.499 * float(w_min(box))
    reach = lambda cutoff, rad: (1.7320508 * cutoff * 1.0005 + 1.0e-3) + rad
    lo_cut = np.float32((limit - 0.05 - 1.0e-3 - radius.max()) / (1.7320508 * 1.0005))
    hi_cut = np.float32((limit + 0.05 - 1.0e-3 - radius.min()) / (1.7320508 * 1.0005))
    assert all(limit - 0.1 < reach(float(lo_cut), r) < limit - 0.02 for r in radius[[np.argmax(radius)]]) and (reach(float(lo_cut), radius) < limit - 0.02).all()
    assert (reach(float(hi_cut), radius) > limit + 0.02).all() and reach(float(hi_cut), radius.min()) < limit + 0.1
    tgt = np.arange(K * m, coords.shape[2], dtype=np.int32)
    for cut in (lo_cut, hi_cut):
        cases.check_sdf(lib, O, coords, box, structures, mass, tgt, float(cut), device=device)


def all_batches():
    """every batch of the direct-call cases: what the 40-digit check of the reference walks over"""
    return slots_batches() + size_batches() + mass_batches() + chain_batches() + [tree_batch()] + cell_batches() + [stride_batch()]
