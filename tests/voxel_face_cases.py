"""Target atoms ON the voxel faces of sdf(): direct calls of vmd_hip_sdf_scatter / vmd_hip_sdf_scatter_masked with R32 and c32 chosen
here, held voxel for voxel (assert_array_equal, u64) against tests/sdf_voxel_ref.py.  For the SIMT emulator (test_voxel_faces_emu.py)
and the product library on the device (test_voxel_faces_gpu.py).  Also here: the three small kernels that turn the u64 accumulators
into what the host sees (vmd_hip_counts_to_float, vmd_hip_axpy_u64, vmd_hip_add_u64).

A case is one launch of B = 3 frames over the same atoms with K = 1 structure: frame 0 under the identity, frame 1 under a signed
permutation, frame 2 under a general rotation rounded to fp32; c32 = (0.337, 0.612, 0.781): a fraction, and positive and below 1 so that the
targets' coordinates have floats at least as fine as q + s has.  Extents: s = 8 (vscale = 8, exact), 10 (vscale = fl(6.4)), 7.

Targets of a frame, all found by searching neighbouring floats with the reference (faces()):
  per axis and k = 0..128: the other two coordinates anywhere inside the cube, this one scanned in 49 steps (a float of the coordinate, or half a float of q + s) around
      c + R^T (k / vscale - s); kept are the target whose t IS k (where a float gives it: for s = 8 that is every k under the
      identity and every k >= 5 under the permutation, asserted), the one with the largest t below k and the one with the smallest t above k.
      k = 0: t = 0 exactly (voxel 0) and the largest reachable t < 0 (out); k = 128: t = dim exactly (out), the largest t < dim (voxel 127).
      t = -0.0 cannot be produced (sdf_voxel_ref's head); test_voxel_faces.py holds the rule on the reference alone.
  the eight corners of the cube: q = +-(1 - e) s on every axis with the smallest e of 1e-6 2^j that the reference still finds inside.
      There |p - c| > 0.99999 sqrt(3) s, next to the reach of the group pre-filter, sqrt(3) s 1.0005 + 1e-3 + group radius.
  atoms whose image is taken: interior targets moved by -1 / 0 / +1 cell edges along the periodic axes.
  the structure's own three atoms (one sits on c32 itself: voxel (64, 64, 64)): skipped, or counted (include_self: `unowned`).
  the rest lies 25 to 29 from c32: outside the reach of any group record.
Cells: a periodic 60 A cube, the same with z open, and 64 x 16 x 64 for targets whose d invL is exactly +-0.5 and +-1.5 on y
(rintf ties to even: 0 and +-2), which under s = 10 lands them in other voxels than rounding half away from zero would.

Group records: NULL (no pre-filter), the one a real vmd_hip_sdf_align call writes for a one-atom structure sitting on c32 (radius
0.01), and the tightest valid one - centre c32, radius 0 - under which a corner target is only 0.0005 sqrt(3) s + 1e-3 inside the reach.
Routes: the list kernel (sdf_ilp 4 / 8 / 16, sdf_wave 0 / 1 / 2), the same over a progression (first 0, stride 1), sdf_rows 1 / 2 / 4,
the dense atom_tag kernel, and the MASKED kernel with a mask that keeps every atom; a word behind every volume is checked."""
import numpy as np

import sdf_voxel_ref as S
from cell_build_cases import Buffers
from geometry_ref import Box
from sdf_align_cases import box9, rot
from test_within import options

f32 = np.float32
DIM, TAIL = 128, 16
SENTINEL = 0x5A5A5A5A5A5A5A5A
CENTRE = np.float32([0.337, 0.612, 0.781])
PERM = np.float32([[0, -1, 0], [0, 0, 1], [-1, 0, 0]])                  # a signed permutation, det +1
GENERAL = rot([0.3, -0.5, 0.8], 67.0).astype(np.float32)
ROTATIONS = (np.eye(3, dtype=np.float32), PERM, GENERAL)


def _steps(x, w):
    """x float32 [n] -> [n, 2 w + 1]: the floats -w..w around each"""
    out = [x]
    lo = hi = x
    for _ in range(w):
        lo, hi = np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf))
        out = [lo] + out + [hi]
    return np.stack(out, axis=1)


def faces(rng, bx, R, c, s, axis, W=24):
    """-> (points float32 [n, 3], exact bool [129]): per k the target on the face and its two neighbours (module head)"""
    vs = float(S.vscale_of(s, DIM))
    k = np.arange(DIM + 1)
    q = rng.uniform(-0.9, 0.9, (k.size, 3)) * float(s)
    q[:, axis] = k / vs - float(s)
    p0 = (c.astype(np.float64) + q @ R.astype(np.float64)).astype(np.float32)          # c + R^T q
    j = int(np.argmax(np.abs(R[axis])))
    cand = np.repeat(p0[:, None, :], 2 * W + 1, axis=1)
    # the scan's step: a float of the coordinate, or half a float of a = q + s where the coordinate's floats are finer than that
    # (under a general rotation q is a rounded sum of three terms of size s: nothing finer than a quarter float of s moves it reliably)
    h = np.maximum(np.spacing(np.abs(p0[:, j])).astype(np.float64), 0.5 * np.spacing((k / vs).astype(np.float32)).astype(np.float64))
    if np.count_nonzero(R) != 3:
        h = np.maximum(h, 0.25 * float(np.spacing(f32(s))))
    cand[:, :, j] = (p0[:, j].astype(np.float64)[:, None] + np.arange(-W, W + 1)[None, :] * h[:, None]).astype(np.float32)
    t = S.t_of(cand.reshape(-1, 3).T, bx, R, c, s, DIM)[0][axis].reshape(k.size, 2 * W + 1)
    kk = k[:, None].astype(np.float32)
    below, above = np.where(t < kk, t, -np.inf), np.where(t > kk, t, np.inf)
    assert np.isfinite(below.max(axis=1)).all() and np.isfinite(above.min(axis=1)).all(), "the scan does not bracket a face"
    pts = [cand[k, below.argmax(axis=1)], cand[k, above.argmin(axis=1)]]
    on = t == kk
    pts.append(cand[k[on.any(axis=1)], on.argmax(axis=1)[on.any(axis=1)]])
    return np.concatenate(pts), on.any(axis=1)


def corners(bx, R, c, s):
    out = []
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            for sz in (-1.0, 1.0):
                for j in range(12):
                    q = np.array([sx, sy, sz]) * float(s) * (1.0 - 1.0e-6 * 2 ** j)
                    p = (c.astype(np.float64) + q @ R.astype(np.float64)).astype(np.float32)
                    if S.in_range(S.t_of(p[:, None], bx, R, c, s, DIM)[0], DIM)[0]:
                        break
                d = np.linalg.norm(S.displacement(p[:, None], bx, c).astype(np.float64))
                assert S.in_range(S.t_of(p[:, None], bx, R, c, s, DIM)[0], DIM)[0] and d > 0.99999 * np.sqrt(3.0) * float(s), (sx, sy, sz, d)
                out.append(p)
    return np.array(out)


class Case:
    """B = 3 frames (one per rotation), K = 1, m = 3; atoms 0..2 are the structure, atom 0 sits on c32"""

    def __init__(self, name, s, edges=(60.0, 60.0, 60.0), pbc=7, seed=1, ties=False):
        self.ties = ties
        self.name, self.s, self.pbc = name, f32(s), pbc
        self.box9 = box9(*edges)
        self.bx = Box(edges, pbc)
        rng = np.random.default_rng(seed)
        L = np.float64(edges)
        per = np.array([bool(pbc & (1 << a)) for a in range(3)])
        frames, self.exact_faces = [], []
        for R in ROTATIONS:
            c = CENTRE
            own = (c.astype(np.float64) + (rng.uniform(-0.8, 0.8, (3, 3)) * float(s)) @ R.astype(np.float64)).astype(np.float32)
            own[0] = c
            pts = [own]
            found = []
            for axis in range(0 if ties else 3):      # the tie cell is narrower than the cube: its faces are not searched
                p, on = faces(rng, self.bx, R, c, s, axis)
                pts.append(p); found.append(on)
            self.exact_faces.append(np.array(found))
            if not ties:
                pts.append(corners(self.bx, R, c, s))
            inner = c.astype(np.float64) + (rng.uniform(-0.95, 0.95, (90, 3)) * float(s)) @ R.astype(np.float64)
            pts.append((inner + np.where(per, rng.integers(-1, 2, (90, 3)), 0) * L).astype(np.float32))
            if ties:            # d invL = +-0.5, +-1.5 exactly on y (L = 16, invL = 2^-4); x and z inside the cube
                for dy in (8.0, -8.0, 24.0, -24.0):
                    p = c.astype(np.float64) + np.array([rng.uniform(-5, 5), 0.0, rng.uniform(-5, 5)])
                    p = p.astype(np.float32)
                    y = _steps(np.float32([c[1] + dy]), 8)[0]
                    y = y[(y - c[1]).astype(np.float32) == f32(dy)]
                    assert y.size, "no float gives the tie"
                    for yy in y[:2]:
                        pts.append(np.float32([[p[0], yy, p[2]]]))
            frames.append(np.concatenate(pts))
        n = max(f.shape[0] for f in frames) + 37
        self.N = N = n + (n % 4 == 0)                                    # a ragged last group of four atoms
        self.rs = (N + 63) // 64 * 64
        self.fs = 3 * self.rs
        self.B, self.K, self.m = len(frames), 1, 3
        self.xyz = np.zeros((self.B, 3, self.rs), np.float32)
        for b, f in enumerate(frames):
            far = rng.normal(size=(N - f.shape[0], 3))
            far = CENTRE + far / np.linalg.norm(far, axis=1)[:, None] * rng.uniform(25.0, 29.0, (far.shape[0], 1))
            self.xyz[b, :, :N] = np.concatenate([f, far.astype(np.float32)]).T
        self.R32 = np.ascontiguousarray(np.stack(ROTATIONS)[:, None], np.float32)          # [B, K, 3, 3]
        self.c32 = np.ascontiguousarray(np.broadcast_to(CENTRE, (self.B, 1, 3)), np.float32)
        self.structs = np.arange(3, dtype=np.int32).reshape(1, 3)
        self.tgt = np.arange(N, dtype=np.int32)
        self._want = {}

    def want(self, include_self):
        if include_self not in self._want:
            vol = np.zeros(DIM ** 3, np.uint64)
            for b in range(self.B):
                S.scatter(self.xyz[b, :, :self.N], self.bx, self.R32[b], self.c32[b], self.tgt, self.s, DIM, self.structs, include_self, vol)
            self._want[include_self] = vol
        return self._want[include_self]


CASES = {
    "s8": dict(s=8.0, seed=11),
    "s10": dict(s=10.0, seed=12),
    "s7": dict(s=7.0, seed=13),
    "s8_open_z": dict(s=8.0, pbc=3, seed=14),
    "s10_ties_on_y": dict(s=10.0, edges=(64.0, 16.0, 64.0), seed=15, ties=True),
}
_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name, **CASES[name])
    return _CASES[name]


def conditions(cs):
    """what the reference says about the case before anything is launched; -> the printed figures"""
    vol, vol_self = cs.want(False), cs.want(True)
    assert int(vol_self.sum()) - int(vol.sum()) == cs.B * cs.m, "the structure's own atoms are not all inside the cube"
    centre = (64 * DIM + 64) * DIM + 64
    assert vol_self[centre] - vol[centre] == cs.B, "the atom on c32 is not in voxel (64, 64, 64)"
    if cs.s == 8.0:
        # under the permutation's minus signs the faces k < 5 lie at p > 8, where the coordinate's floats are coarser than those of q + s
        assert cs.exact_faces[0].all() and cs.exact_faces[1][:, 5:].all(), "s = 8: a face of the identity / the permutation has no target exactly on it"
    fig = dict(exact=[int(e.sum()) for e in cs.exact_faces])
    worst, differ, near, flips = 0.0, 0, 0, 0
    for b in range(cs.B):
        t, d = S.t_of(cs.xyz[b, :, :cs.N], cs.bx, cs.R32[b, 0], cs.c32[b, 0], cs.s, DIM)
        close = np.linalg.norm(d.astype(np.float64), axis=0) < 20.0
        for a in range(0 if cs.ties else 3):               # both sides of 0 and of dim are met, and both voxels of every inner face
            ta = t[a, close]
            assert (ta < 0).any() and (ta == 0).any() == bool(cs.exact_faces[b][a, 0]) and (ta >= DIM).any()
            v = np.trunc(ta[(ta >= 0) & (ta < DIM)]).astype(int)
            assert np.bincount(v, minlength=DIM).min() >= 1, f"{cs.name}: frame {b}, axis {a}: a voxel layer has no target"
        c = S.compare(cs.xyz[b, :, :cs.N][:, close], cs.bx, cs.R32[b, 0], cs.c32[b, 0], cs.s, DIM, what=f"{cs.name} frame {b}")
        worst, differ, near, flips = max(worst, c["worst"]), differ + c["differ"], near + c["near"], flips + c["flips"]
    if cs.ties:           # ties to even leave +-8 where it is and take two edges off +-24; half away from zero would give -+8 both times
        for b in range(cs.B):
            d = S.displacement(cs.xyz[b, :, :cs.N], cs.bx, cs.c32[b, 0])
            assert int((d[1] == f32(8.0)).sum()) >= 2 and int((d[1] == f32(-8.0)).sum()) >= 2
    fig.update(N=cs.N, inside=int(vol.sum()), differ=differ, near=near, flips=flips, worst=worst)
    print(f"voxel_faces {cs.name}: N = {cs.N}, {fig['inside']} of {cs.B} x {cs.N} targets inside; faces with a target exactly on them (of 3 x 129): "
          f"identity {fig['exact'][0]}, permutation {fig['exact'][1]}, general {fig['exact'][2]}; coordinates within the exact margin of a face "
          f"{near}, fp32 voxel != exact voxel {differ} (worst offset {worst:.3f} of its margin), in for one tier and out for the other {flips}")
    return fig


# ---- the launches -----------------------------------------------------------------------------------------------------------------------

BASE = dict(sdf_wave=0, sdf_ilp=4, sdf_rows=0, sdf_nt=0)
# name -> (target form, options)
ROUTES = {
    "list": ("list", {}), "list_ilp8": ("list", dict(sdf_ilp=8)), "list_ilp16": ("list", dict(sdf_ilp=16)),
    "list_wave1": ("list", dict(sdf_wave=1)), "list_wave1_ilp8": ("list", dict(sdf_wave=1, sdf_ilp=8)), "list_wave2": ("list", dict(sdf_wave=2)),
    "list_nt": ("list", dict(sdf_nt=1)),
    "progression": ("arith", {}), "progression_ilp8": ("arith", dict(sdf_ilp=8)), "progression_wave1": ("arith", dict(sdf_wave=1)),
    "progression_wave2": ("arith", dict(sdf_wave=2)),
    "rows1": ("arith", dict(sdf_rows=1)), "rows2": ("arith", dict(sdf_rows=2)), "rows4": ("arith", dict(sdf_rows=4)),
    "dense": ("dense", {}),
    "masked_list": ("masked_list", {}), "masked_progression": ("masked_arith", {}), "masked_list_ilp8": ("masked_list", dict(sdf_ilp=8)),
}
GROUPS = ("none", "aligned", "tight")
OWNERS = ("owner", "search", "include_self")


def aligned_group(lib, cs, gpu):
    """the group record of a real vmd_hip_sdf_align call: a one-atom structure, atom 0, which sits on c32"""
    nan = lambda n, t: np.full(n, np.nan, t)
    buf = Buffers(gpu, xyz=cs.xyz.reshape(-1), boxes=np.tile(cs.box9, cs.B), structs=np.zeros(1, np.int32), pose=nan(3 + TAIL, np.float64),
                  R32=nan(9 * cs.B + TAIL, np.float32), c32=nan(3 * cs.B + TAIL, np.float32), group=nan(4 * cs.B + TAIL, np.float32))
    assert lib.vmd_hip_sdf_ref_pose(None, buf["xyz"], cs.rs, buf["boxes"], cs.pbc, buf["structs"], None, 1, buf["pose"], None, None) == 0
    assert lib.vmd_hip_sdf_align(None, buf["xyz"], cs.fs, cs.rs, buf["boxes"], cs.pbc, cs.B, buf["structs"], None, 1, 1, buf["pose"],
                                 buf["R32"], buf["c32"], None, buf["group"], None, None, None) == 0
    g = buf.fetch("group").copy()
    assert np.isnan(g[4 * cs.B:]).all()
    g = g[:4 * cs.B].reshape(cs.B, 4)
    np.testing.assert_array_equal(g[:, :3].view(np.uint32), cs.c32[:, 0].view(np.uint32), err_msg="the aligned centre is not the atom on c32")
    assert (g[:, 3] == f32(0.01)).all()
    return g


def launch(lib, cs, gpu, route, group="none", owner="owner", aligned=None):
    form, opts = ROUTES[route]
    masked, form = form.startswith("masked_"), form.replace("masked_", "")
    include_self = owner == "include_self"
    vol = np.zeros(DIM ** 3 + TAIL, np.int64)
    vol[DIM ** 3:] = SENTINEL
    own = np.where(cs.tgt < cs.m, 0, -1).astype(np.int8)
    tag = np.full(cs.rs, 255, np.uint8)
    tag[:cs.N] = 254
    if not include_self:
        tag[:cs.m] = 0
    g = None if group == "none" else aligned if group == "aligned" else np.concatenate([cs.c32[:, 0], np.zeros((cs.B, 1), np.float32)], axis=1)
    buf = Buffers(gpu, xyz=cs.xyz.reshape(-1), boxes=np.tile(cs.box9, cs.B), structs=cs.structs.reshape(-1), R32=cs.R32.reshape(-1),
                  c32=cs.c32.reshape(-1), tgt=cs.tgt if form == "list" else None, owner=own if owner == "owner" else None, vol=vol,
                  group=None if g is None else np.ascontiguousarray(g, np.float32).reshape(-1), tag=tag if form == "dense" else None,
                  mask=np.ones(cs.B * cs.rs, np.uint8) if masked else None)
    stride = 0 if form == "list" else 1
    with options(lib, **{**BASE, **opts}):
        if masked:
            rc = lib.vmd_hip_sdf_scatter_masked(None, buf["xyz"], cs.fs, cs.rs, buf["boxes"], cs.pbc, cs.B, buf["structs"], cs.K, cs.m, buf["R32"],
                                                buf["c32"], buf["tgt"], buf["owner"], cs.N, float(cs.s), DIM, buf["vol"], buf["group"], 0, stride,
                                                1 if include_self else 0, buf["mask"], cs.rs, None)
        else:
            rc = lib.vmd_hip_sdf_scatter(None, buf["xyz"], cs.fs, cs.rs, buf["boxes"], cs.pbc, cs.B, buf["structs"], cs.K, cs.m, buf["R32"],
                                         buf["c32"], buf["tgt"], buf["owner"], cs.N, float(cs.s), DIM, buf["vol"], buf["group"], buf["tag"], 0, stride,
                                         1 if include_self else 0)
        assert rc == 0, rc
        out = buf.fetch("vol").view(np.uint64)
    assert (out[DIM ** 3:] == np.uint64(SENTINEL)).all(), f"{cs.name} {route}: the words behind the volume were written"
    return out[:DIM ** 3]


def run(lib, name, route, device=False):
    cs = case(name)
    aligned = aligned_group(lib, cs, device)
    for group in GROUPS:
        got = launch(lib, cs, device, route, group, "owner", aligned)
        np.testing.assert_array_equal(got, cs.want(False), err_msg=f"{name} {route}: group record {group}")
    for owner in OWNERS[1:]:
        got = launch(lib, cs, device, route, "tight", owner, aligned)
        np.testing.assert_array_equal(got, cs.want(owner == "include_self"), err_msg=f"{name} {route}: tight group record, {owner}")


# ---- the accumulators' small kernels ----------------------------------------------------------------------------------------------------

SIZES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, DIM ** 3)
SPECIAL = np.array([0, 1, 2 ** 24 - 1, 2 ** 24 + 1, 2 ** 32 + 1, 2 ** 53 + 1], np.uint64)
DENSITY = np.float32(1.0 / (7 * (2.0 * 10.0 / DIM) ** 3))               # spec_sdf_density: 7 frames, s = 10


def _counts(n, seed, zero=False):
    rng = np.random.default_rng(seed)
    c = np.zeros(n, np.uint64) if zero else rng.integers(0, 5, n).astype(np.uint64)
    if not zero:
        at = rng.permutation(n)[:SPECIAL.size]
        c[at] = SPECIAL[:at.size] if n >= SPECIAL.size else SPECIAL[-at.size:]
        c[n - 1] = SPECIAL[(n + seed) % SPECIAL.size]
    return c


def _rne32(v):
    """the fp32 number nearest to the integer v, ties to even, in integer arithmetic"""
    shift = max(0, v.bit_length() - 24)
    q, rem = v >> shift, v & ((1 << shift) - 1)
    if shift and (rem > (1 << (shift - 1)) or (rem == (1 << (shift - 1)) and q & 1)):
        q += 1
    return np.float32(float(q) * 2.0 ** shift)                   # q <= 2^24: both factors and the product are exact


def to_f32(counts):
    """(float)u64 with one rounding to nearest even"""
    u = np.unique(counts)
    return np.array([_rne32(int(v)) for v in u], np.float32)[np.searchsorted(u, counts)]


def counts_to_float(lib, n, device=False):
    for zero in (False, True):
        for scale in (np.float32(1.0), DENSITY):
            c = _counts(n, n % 1000 + 1, zero)
            vals = np.full(n + TAIL, np.nan, np.float32)
            mx = np.full(1 + TAIL, np.nan, np.float32)
            buf = Buffers(device, c=c.view(np.int64), v=vals, m=mx)
            assert lib.vmd_hip_counts_to_float(None, buf["c"], n, buf["v"], buf["m"], float(scale)) == 0
            v, m = buf.fetch("v").copy(), buf.fetch("m").copy()
            want = (to_f32(c) * scale).astype(np.float32)
            np.testing.assert_array_equal(v[:n].view(np.uint32), want.view(np.uint32), err_msg=f"n = {n}, scale = {scale}")
            assert np.isnan(v[n:]).all() and np.isnan(m[1:]).all(), f"n = {n}: a word behind an output was written"
            assert m[0] == (want.max() if not zero else 0.0), (n, m[0], want.max())
            if not zero:                                          # max_out == NULL: accepted, same values
                buf = Buffers(device, c=c.view(np.int64), v=vals)
                assert lib.vmd_hip_counts_to_float(None, buf["c"], n, buf["v"], None, float(scale)) == 0
                np.testing.assert_array_equal(buf.fetch("v")[:n].view(np.uint32), want.view(np.uint32))


def axpy_add(lib, n, device=False):
    src, dst0 = _counts(n, n % 1000 + 2), _counts(n, n % 1000 + 3)
    src[::3] = 0                                                  # the kernels skip zero sources
    guard = np.full(TAIL, SENTINEL, np.uint64)
    for mult in (0, 1, 3):
        for flag in (None, 0, 1):
            buf = Buffers(device, d=np.concatenate([dst0, guard]).view(np.int64), s=src.view(np.int64),
                          f=None if flag is None else np.array([flag, 7], np.int32))
            assert lib.vmd_hip_axpy_u64(None, buf["d"], buf["s"], n, mult, buf["f"]) == 0
            got = buf.fetch("d").view(np.uint64)
            want = dst0 if flag == 1 else dst0 + np.uint64(mult) * src
            np.testing.assert_array_equal(got[:n], want, err_msg=f"axpy n = {n}, mult = {mult}, skip flag {flag}")
            assert (got[n:] == guard).all(), f"axpy n = {n}: the words behind dst were written"
    buf = Buffers(device, d=np.concatenate([dst0, guard]).view(np.int64), s=src.view(np.int64))
    assert lib.vmd_hip_add_u64(None, buf["d"], buf["s"], n) == 0
    got = buf.fetch("d").view(np.uint64)
    np.testing.assert_array_equal(got[:n], dst0 + src, err_msg=f"add n = {n}")
    assert (got[n:] == guard).all(), f"add n = {n}: the words behind dst were written"
