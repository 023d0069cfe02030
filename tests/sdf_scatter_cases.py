"""The SDF scatter kernels (K4: k_sdf_scatter static and MASKED, _wave, _stream, _rows, _dense) at their size edges: the systems and the
routes, run by tests/test_sdf_scatter_emu.py on the SIMT emulator and by tests/test_sdf_scatter_gpu.py on the device.

Voxel counts are integers: every comparison is assert_array_equal against the oracle's sdf_frame_scatter (cases.oracle_sdf; through
tests/shell_sdf_ref.py for the MASKED route, whose target is a shell).  The oracle's volume is computed once per system and every route
is held against it - it does not depend on a switch.

A system is built so that the number of survivors of the group test (vmd_sdf_near) is known per (frame, tile): open boundaries, K
structures around CENTRE, `n_near` targets inside a ball of radius 10 around structure 0, every other target farther than 40 from it;
the reach of the test is 1.7321 * 10 * 1.0005 + 1e-3 + the group radius (0.01 for K = 1) = 17.34.  build() counts both sets on the CPU
from the fp32 coordinates and asserts them.  `near` holds SLOTS of the target list: slot t sits in block t / (256 ILP), and in the
wave kernels in wave tile t / (64 ILP), lane t % 64, register u = t / 64 % ILP."""
import numpy as np

import viamd_amd as V

import cases
import shell_sdf_ref as S
from test_within import evaluate, options

BOX, CUTOFF, DIM = 400.0, 10.0, 128
CENTRE = np.array([200.0, 200.0, 200.0])
N_S = 6                                     # atoms of the one structure of a K = 1 system: the targets start behind it
SHELL = 0.05                                # MASKED: a marker atom sits 0.01 from every second near atom, the shell is within(0.05, markers)


class System:
    def __init__(self, coords, structures, mass, tgt, near, markers):
        self.coords, self.structures, self.mass, self.tgt, self.near, self.markers = coords, structures, mass, tgt, near, markers
        self._want = {}

    def want(self, O, masked=False):
        """the oracle's volume, once"""
        if masked not in self._want:
            if masked:
                vol, pops = S.shell_sdf(O, self.coords, BOX, self.structures, self.mass, (self.tgt, (self.markers, 0.0, SHELL)), CUTOFF, flags=0)
                kept = (self.near.size + 1) // 2
                assert pops.tolist() == [kept] * self.coords.shape[0], (pops, kept)      # the shell keeps every second near atom, nothing else
            else:
                vol = cases.oracle_sdf(O, self.coords, cases.cell_pair(O, BOX, 0)[0], self.structures, self.mass, self.tgt, CUTOFF, DIM)[0]
            assert (vol.sum() > 0) == (self.near.size > 0)
            self._want[masked] = vol
        return self._want[masked]


def _directions(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def build(seed, tgt, near, N, K=1, m=N_S, frames=2, markers=False):
    """tgt: atom index per target slot; near: the slots whose atoms lie near the structures (atoms of the structures among the targets
    must be listed: they are near).  Atoms [0, K m) are the structures.  markers: N grows by one atom per second near target (MASKED)."""
    rng = np.random.default_rng(seed)
    tgt, near = np.asarray(tgt, np.int32), np.asarray(sorted(set(int(s) for s in near)), np.int64)
    n_s = K * m
    free = near[tgt[near] >= n_s]                                    # near targets that are not structure atoms
    marked = tgt[near][::2] if markers else np.zeros(0, np.int32)
    assert not markers or (free.size == near.size and near.size <= tgt.size)
    mk = np.arange(N, N + max(1, marked.size), dtype=np.int32) if markers else None
    N_all = N + (mk.size if markers else 0)
    pos = CENTRE + _directions(rng, N_all) * rng.uniform(50.0, 80.0, (N_all, 1))           # everything far ...
    pos[tgt[free]] = CENTRE + _directions(rng, free.size) * (8.0 * rng.uniform(0.0, 1.0, (free.size, 1)) ** (1.0 / 3.0))   # ... but these
    template = rng.normal(0.0, 1.2, (m, 3))
    offsets = _directions(rng, K) * rng.uniform(0.2, 0.9, (K, 1))   # centres within 2 of each other
    offsets[0] = 0.0
    coords = np.zeros((frames, 3, N_all), np.float32)
    for f in range(frames):
        p = pos + rng.normal(0.0, 0.05, pos.shape)
        for k in range(K):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            q = q * np.sign(np.linalg.det(q))
            p[k * m:(k + 1) * m] = template @ q.T + CENTRE + offsets[k] + rng.normal(0.0, 0.1, 3)
        if markers and marked.size:
            p[mk] = p[marked] + (0.01, 0.0, 0.0)
        coords[f] = p.T.astype(np.float32)
    structures = np.arange(n_s, dtype=np.int32).reshape(K, m)
    mass = np.ones(N_all, np.float32)
    mass[:n_s] = rng.choice([12.011, 14.007, 15.999, 1.008], n_s).astype(np.float32)
    # the survivors of the group test, from the fp32 coordinates: |x - c_0| against reach, c_k the mass-weighted centres
    for f in range(frames):
        x = coords[f].astype(np.float64).T
        com = np.array([np.average(x[s], axis=0, weights=mass[s].astype(np.float64)) for s in structures])
        reach = 1.7320508 * CUTOFF * 1.0005 + 1.0e-3 + np.linalg.norm(com - com[0], axis=1).max() * 1.0005 + 1.0e-2
        assert 17.34 <= reach + 5.0e-3 and reach < 20.0, reach
        d = np.linalg.norm(x[tgt] - com[0], axis=1)
        assert np.array_equal(np.nonzero(d < 10.0)[0], near) and int((d > 40.0).sum()) == tgt.size - near.size, (f, near.size)
    return System(coords, structures, mass, tgt, near, mk)


def progression(ntgt, first=N_S, stride=3):
    """-> (tgt, N): first + stride t, the trajectory ends with the last target"""
    tgt = first + stride * np.arange(ntgt, dtype=np.int32)
    return tgt, int(tgt[-1]) + 1


def irregular(seed, ntgt):
    """-> (tgt, N): a sorted list that is no progression"""
    N = N_S + 3 * ntgt + 7
    tgt = np.sort(np.random.default_rng(seed).choice(np.arange(N_S, N, dtype=np.int32), ntgt, replace=False)).astype(np.int32)
    if ntgt >= 3 and np.all(np.diff(tgt) == tgt[1] - tgt[0]):
        tgt[-1] = N - 1 if tgt[-1] != N - 1 else N - 2
    return tgt, N


def some(seed, ntgt, n, lo=0, hi=None):
    """n slots of [lo, hi), the first and the last one among them"""
    hi = ntgt if hi is None else min(hi, ntgt)
    n = min(n, hi - lo)
    if n <= 0:
        return np.zeros(0, np.int64)
    pick = set([lo, hi - 1][:n])
    rest = np.array([s for s in range(lo, hi) if s not in pick])
    pick.update(np.random.default_rng(seed).choice(rest, n - len(pick), replace=False).tolist())
    return np.array(sorted(pick))


def product(lib, sy, device, masked=False, **opts):
    with options(lib, **opts):                  # restores every switch on the way out, whatever happens
        ir = V.ScriptIR(lib)
        if masked:
            ir.add_sdf_shell("v", sy.structures, sy.tgt, CUTOFF, target_shell=(sy.markers, 0.0, SHELL))
        else:
            ir.add_sdf("v", sy.structures, sy.tgt, CUTOFF)
        ev = evaluate(lib, ir, sy.coords, BOX, flags=0, device=device, mass=sy.mass)
        pd = ev.property_data("v")
        assert tuple(pd.dim)[1:] == (DIM, DIM, DIM)
        return np.array(pd.counts, copy=True)


def hold(lib, O, sy, device, what, masked=False, **opts):
    route = dict(sdf_arith=1, sdf_ilp=4, sdf_wave=0, sdf_rows=0, sdf_dense=0, sdf_nt=0)
    route.update(opts)
    np.testing.assert_array_equal(product(lib, sy, device, masked, **route), sy.want(O, masked), err_msg=f"{what} {opts}")


# ---- the cases ------------------------------------------------------------------------------------------------------------------------

TARGET_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)      # ILP 4: block tile 1 024, wave tile 256
ILP_COUNTS = (2047, 2049, 4097)                                             # ILP 8 / 16: block tiles 2 048 / 4 096, wave tile 512


def target_count(lib, O, ntgt, device=False):
    """list and progression over every list kernel, the last target of a ragged tile near"""
    tgt, N = progression(ntgt)
    sy = build(100 + ntgt, tgt, some(ntgt, ntgt, 5), N)
    for wave in (0, 1, 2):
        hold(lib, O, sy, device, f"progression {ntgt}", sdf_wave=wave)
    hold(lib, O, sy, device, f"progression as a list {ntgt}", sdf_arith=0)
    tgt, N = irregular(ntgt, ntgt)
    sy = build(200 + ntgt, tgt, some(ntgt + 1, ntgt, 5), N)
    for wave in (0, 1, 2):
        hold(lib, O, sy, device, f"irregular list {ntgt}", sdf_wave=wave)


def ilp_target_count(lib, O, ntgt, device=False):
    tgt, N = progression(ntgt)
    sy = build(300 + ntgt, tgt, some(ntgt, ntgt, 9), N)
    for arith in (0, 1):
        for ilp, wave in ((8, 0), (8, 1), (8, 2), (16, 0)):
            hold(lib, O, sy, device, f"{ntgt} targets", sdf_arith=arith, sdf_ilp=ilp, sdf_wave=wave)


BLOCK_NEAR = (0, 1, 511, 512, 513, 1024)    # among the 1 024 targets of one block: VMD_SDF_CAP = 512 a round


def block_rounds(lib, O, n_near, device=False):
    """one block of k_sdf_scatter (static and MASKED) and the blocks of k_sdf_scatter_rows: no round, one, one full, two, two full"""
    tgt, N = progression(1024)
    sy = build(400 + n_near, tgt, some(n_near, 1024, n_near), N, markers=True)
    for arith in (0, 1):
        hold(lib, O, sy, device, f"block, {n_near} near", sdf_arith=arith)
        hold(lib, O, sy, device, f"masked block, {n_near} near", masked=True, sdf_arith=arith)
    for rows in (1, 2, 4):
        hold(lib, O, sy, device, f"rows, {n_near} near", sdf_rows=rows)


WAVE_NEAR = (0, 1, 63, 64, 65, 129, 256)    # among the 256 targets of ONE wave (the second of its block): 64 slots a round


def wave_rounds(lib, O, n_near, device=False):
    tgt, N = progression(1024)
    if n_near == 65:
        near = np.concatenate([np.arange(256 + 64, 256 + 128), [256 + 128 + 17]])      # register u = 1 of every lane: one full ballot, and one more
    else:
        near = some(n_near, 1024, n_near, lo=256, hi=512)
    sy = build(500 + n_near, tgt, near, N)
    for wave in (1, 2, 16):
        for arith in (0, 1):
            hold(lib, O, sy, device, f"wave, {n_near} near", sdf_wave=wave, sdf_arith=arith)


# sdf_wave = 16: 16 blocks = 64 waves walk tiles_per_frame * B tiles.  (ntgt, frames) -> tiles: 6 (most waves return at once, a partial
# block), 64, 65 (one wave ends on its second register set), 129 (one wave ends on the first again: 43 tiles x 3 frames)
STREAM_WALKS = ((700, 2), (4096, 4), (3300, 5), (11008, 3))


def stream_walk(lib, O, ntgt, frames, device=False):
    tgt, N = progression(ntgt)
    sy = build(600 + ntgt, tgt, some(ntgt, ntgt, 40), N, frames=frames)
    for arith in (0, 1):
        hold(lib, O, sy, device, f"stream, {ntgt} x {frames}", sdf_wave=16, sdf_arith=arith, batch_frames=8)


def rows_shapes(lib, O, device=False):
    """k_sdf_scatter_rows: where the first target sits in its group of 4 atoms, every stride (5: the route falls back to the block
    kernel), 255 / 256 / 257 groups for one group per thread, and a last group that the trajectory ends in"""
    shapes = [(N_S + d, 3, 300) for d in range(4)] + [(N_S, s, 300) for s in (1, 2, 4, 5)] + [(8, 4, n) for n in (255, 256, 257)] + [(8, 3, 301)]
    for first, stride, ntgt in shapes:
        tgt, N = progression(ntgt, first, stride)
        sy = build(700 + 16 * first + stride + ntgt, tgt, some(first + stride, ntgt, 20), N)
        for rows in (1, 2, 4):
            hold(lib, O, sy, device, f"rows: first {first}, stride {stride}, {ntgt} targets", sdf_rows=rows)


def dense_shapes(lib, O, device=False):
    """k_sdf_scatter_dense reads whole groups of 4 atoms: 255, 256, 257 groups hold atoms (a row itself is padded to 64 atoms, so the
    grid covers 256, 256 and 272 groups), the targets are every third atom"""
    for N in (1020, 1024, 1028):
        tgt = np.arange(N_S, N, 3, dtype=np.int32)
        sy = build(800 + N, tgt, some(N, tgt.size, 20), N)
        hold(lib, O, sy, device, f"dense, {N} atoms", sdf_dense=1)


ROUTES = (dict(), dict(sdf_arith=0), dict(sdf_ilp=8), dict(sdf_ilp=16), dict(sdf_wave=1), dict(sdf_wave=2), dict(sdf_wave=16),
          dict(sdf_rows=1), dict(sdf_rows=4), dict(sdf_dense=1))


def seven_structures(lib, O, device=False):
    """K = 7: 37 and 530 survivors make 259 and 3 710 (survivor, structure) pairs - no multiple of 64 or 256"""
    tgt, N = progression(1500, first=35)
    for n_near in (37, 530):
        sy = build(900 + n_near, tgt, some(n_near, 1024, n_near), N, K=7, m=5, markers=True)
        for route in ROUTES:
            hold(lib, O, sy, device, f"K = 7, {n_near} near", **route)
        hold(lib, O, sy, device, f"K = 7 masked, {n_near} near", masked=True)


def own_atoms(lib, O, device=False):
    """the targets include the structures' own atoms (D-SDF-EXCL): every atom is a target"""
    K, m, N = 3, 4, 1500
    tgt = np.arange(N, dtype=np.int32)
    sy = build(1000, tgt, np.concatenate([np.arange(K * m), some(3, N, 30, lo=K * m)]), N, K=K, m=m)
    for route in ROUTES:
        hold(lib, O, sy, device, "own atoms", **route)
