"""The cell build (K1) at its size edges, build by build: vmd_hip_cells_build (atomic k_cells_count / _scan / _scatter, k_cells_fused,
k_cells_split_*) and vmd_hip_cells_build_pencil (k_cells_bin or k_cells_bin_sorted, then k_cells_pen_scan + k_cells_pen_sort) called
directly with a grid of the case's own choosing; run by tests/test_cell_build_emu.py on the SIMT emulator and by
tests/test_cell_build_gpu.py on the device.

What is held, bit for bit, for every frame b: cell_start[b] is the exclusive prefix of bincount(cell) with cell_start[b][ncell] == nsel,
and the triples of sorted[b][:, cs[c]:cs[c + 1]] are the reference's wrapped triples of cell c as a multiset (both sides ordered by their
bit patterns inside the cell: the order there is arbitrary in every build).  Padding beyond nsel is not looked at.

The reference is not the code under test: wrapped coordinates from the oracle's vo_wrap (open axes pass through), the cell index from a
float32 NumPy restatement of vmd_cell_coord - min(max(int32(u * (float32(n) * iL)), 0), n - 1), every product in float32, u the wrapped
coordinate (periodic axis) or x - origin (open axis: extent, inverse extent and origin in the nine-float box as the evaluator and
test_shell_sdf.kernel_masks prepare them).  Triclinic cells stay with the end-to-end RDF cases (their wrap needs chained fmaf).

Every system carries atoms on the faces: the origin, -0.0, nextafter(L, 0) on all axes (the last cell of the table), x = L exactly, whole
multiples of the cell edge on every axis, and one atom a million boxes away from another."""
import ctypes as C

import numpy as np

from viamd_amd import _lib as L

from test_within import options

BOX = np.float32([50.0, 40.0, 30.0])
GARBAGE = 0xdeadbeef


def grid3(nxf, ny, nz):
    return L.Grid(nxf, ny, nz, nxf * ny * nz)


def grid_of(ncell):
    """ncell cells cut as evenly as its divisors allow: tables of any length, primes included"""
    nz = max(d for d in range(1, int(round(ncell ** (1.0 / 3.0))) + 1) if ncell % d == 0)
    rest = ncell // nz
    ny = max(d for d in range(1, int(rest ** 0.5) + 1) if rest % d == 0)
    return grid3(rest // ny, ny, nz)


def grid_of_pencils(npen, nxf=3):
    ny = max(d for d in range(1, int(npen ** 0.5) + 1) if npen % d == 0)
    return grid3(nxf, npen // ny, ny)


# ---- selections: atoms + the form the build is told them in ---------------------------------------------------------------------------

class Sel:
    def __init__(self, atoms, form="list", pattern=None):
        self.atoms, self.form, self.pattern = np.ascontiguousarray(atoms, np.int32), form, pattern


def sel_list(seed, nsel, N):
    return Sel(np.sort(np.random.default_rng(seed).choice(N, nsel, replace=False)))


def sel_forms(N):
    """absent (every atom), an explicit list, and the two computed forms: the O of every water (m = 1), the two H (m = 2)"""
    w = N // 3
    return [Sel(np.arange(N), "absent"),
            sel_list(N, N // 2 + 1, N),
            Sel(2 + 3 * np.arange(w - 1), "pattern", (1, 2, 3, (0, 0, 0, 0))),
            Sel((3 * np.arange(w)[:, None] + np.array([1, 2])[None, :]).ravel(), "pattern", (2, 0, 3, (1, 2, 0, 0)))]


# ---- systems and their reference --------------------------------------------------------------------------------------------------------

class System:
    def __init__(self, seed, N, B, grid, sel, flags=7, pencil=None):
        rng = np.random.default_rng(seed)
        n = (grid.nxf, grid.ny, grid.nz)
        c = (rng.uniform(-1.0, 2.0, (B, 3, N)) * BOX[None, :, None]).astype(np.float32)
        if pencil is not None:                                       # every atom strictly inside pencil (cy, cz)
            for a, k in ((1, pencil[0]), (2, pencil[1])):
                c[:, a, :] = ((k + rng.uniform(0.1, 0.9, (B, N))) * float(BOX[a]) / n[a]).astype(np.float32)
        else:
            self._plant(rng, c, sel.atoms, n, flags)
        self.coords, self.flags, self.grid, self.sel = c, flags, grid, sel
        g9 = np.tile(np.concatenate([BOX, np.float32(1.0) / BOX, np.zeros(3, np.float32)]).astype(np.float32), (B, 1))
        for a in range(3):
            if not (flags >> a) & 1:      # an open axis: extent, inverse extent and origin of the batch's bounding box
                lo, hi = np.float32(c[:, a].min()), np.float32(c[:, a].max())
                pad = np.float32(max(1.0e-2, 1.0e-3 * float(hi - lo)))
                g9[:, 6 + a] = lo - pad; g9[:, a] = (hi - lo) + np.float32(2.0) * pad; g9[:, 3 + a] = np.float32(1.0) / g9[0, a]
        self.g9 = np.ascontiguousarray(g9, np.float32)
        self._ref = None

    @staticmethod
    def _plant(rng, c, atoms, n, flags):
        """the face atoms (values of cases.rdf_edge_cases), on atoms of the selection, in every frame"""
        faces = [{0: 0.0, 1: 0.0, 2: 0.0}, {0: -0.0, 1: -0.0, 2: -0.0},
                 {a: np.nextafter(BOX[a], np.float32(0)) for a in range(3)}]
        for a in range(3):
            faces.append({a: BOX[a]})                                # exactly on the far face (wraps to 0)
            for k in sorted({1, n[a] // 2, n[a] - 1} - {0}):
                faces.append({a: np.float32(k) * (BOX[a] / np.float32(n[a]))})
        slots = rng.permutation(atoms.size)[:len(faces) + 2]
        for s, f in zip(slots, faces):
            for a, v in f.items():
                c[:, a, atoms[s]] = np.float32(v)
        if flags == 7 and slots.size == len(faces) + 2:              # far outside the cell: the image of another atom
            c[:, :, atoms[slots[-1]]] = c[:, :, atoms[slots[-2]]] + np.float32(1.0e6) * BOX[None, :]

    def reference(self, O):
        """-> (wrapped triples f32[B][3][nsel], cell i64[B][nsel]), once"""
        if self._ref is None:
            wrap = O.lib().vo_wrap
            atoms, g = self.sel.atoms, self.grid
            B = self.coords.shape[0]
            n, mul = (g.nxf, g.ny, g.nz), (1, g.nxf, g.nxf * g.ny)
            xyz, cell = np.empty((B, 3, atoms.size), np.float32), np.zeros((B, atoms.size), np.int64)
            for b in range(B):
                for a in range(3):
                    x = self.coords[b, a, atoms]
                    Lf, iL = self.g9[b, a], self.g9[b, 3 + a]
                    if (self.flags >> a) & 1:
                        x = u = np.array([wrap(float(v), float(Lf)) for v in x], np.float32)
                    else:
                        u = x - self.g9[b, 6 + a]
                    xyz[b, a] = x
                    cc = (u * (np.float32(n[a]) * iL)).astype(np.int32)
                    cell[b] += mul[a] * np.minimum(np.maximum(cc, 0), n[a] - 1).astype(np.int64)
            assert u.dtype == np.float32 and 0 <= cell.min() and cell.max() < g.ncell
            self._ref = xyz, cell
        return self._ref


def held(sy, O, cs, srt, what):
    ref_xyz, ref_cell = sy.reference(O)
    B, _, nsel = ref_xyz.shape
    ncell = sy.grid.ncell
    cs, srt = cs.reshape(B, ncell + 1), srt[:B * 3 * ((nsel + 63) & ~63)].reshape(B, 3, -1)
    for b in range(B):
        counts = np.bincount(ref_cell[b], minlength=ncell)
        want = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
        assert want[ncell] == nsel
        np.testing.assert_array_equal(cs[b], want, err_msg=f"cell_start, frame {b}: {what}")
        slot_cell = np.repeat(np.arange(ncell), counts)
        got, ref = srt[b][:, :nsel].view(np.uint32), ref_xyz[b].view(np.uint32)
        gi, ri = np.lexsort((got[2], got[1], got[0], slot_cell)), np.lexsort((ref[2], ref[1], ref[0], ref_cell[b]))
        np.testing.assert_array_equal(got[:, gi], ref[:, ri], err_msg=f"sorted, frame {b}: {what}")


# ---- the calls ------------------------------------------------------------------------------------------------------------------------------

class Buffers:
    """host arrays, or their copies in device memory (torch, as test_shell_sdf.kernel_masks takes it)"""

    def __init__(self, gpu, **host):
        self.gpu, self.host = gpu, {k: v for k, v in host.items() if v is not None}
        if gpu:
            import torch
            self.torch = torch
            self.dev = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in self.host.items()}
            torch.cuda.synchronize()

    def __getitem__(self, k):
        if k not in self.host:
            return None
        return self.dev[k].data_ptr() if self.gpu else self.host[k].ctypes.data

    def fetch(self, k):
        if not self.gpu:
            return self.host[k]
        self.torch.cuda.synchronize()
        return self.dev[k].cpu().numpy().view(self.host[k].dtype)


class pattern_of:
    """the thread's selection pattern for the length of a with block"""

    def __init__(self, lib, sel):
        self.lib, self.pattern = lib, sel.pattern

    def __enter__(self):
        if self.pattern:
            m, first, period, off = self.pattern
            self.lib.vmd_hip_set_cells_sel_pattern(m, first, period, (C.c_int32 * 4)(*off))

    def __exit__(self, *exc):
        self.lib.vmd_hip_set_cells_sel_pattern(0, 0, 0, None)


def _common(sy):
    B, _, N = sy.coords.shape
    nsel = int(sy.sel.atoms.size)
    npad = (nsel + 63) & ~63
    assert sy.sel.form != "absent" or nsel == N
    host = dict(xyz=sy.coords, g9=sy.g9, sel=sy.sel.atoms if sy.sel.form == "list" else None,
                cs=np.full(B * (sy.grid.ncell + 1), GARBAGE, np.uint32), srt=np.full(B * 3 * npad + 64, np.nan, np.float32))
    return B, N, nsel, npad, host


SINGLE = dict(atomic=dict(cells_fused=0, cells_split=1), fused=dict(cells_fused=1, cells_split=1), split=dict(cells_fused=1, cells_split=2),
              split1024=dict(cells_fused=1, cells_split=1024), default=dict())
SLICE = dict(split=2048, split1024=1024)
ROUTE = dict(atomic="atomic", fused="fused", split="split", split1024="split", default="atomic")     # the kernels that must run


def single(lib, O, sy, build, gpu=False):
    """vmd_hip_cells_build through `build`, with the AoS staging buffer and without it"""
    B, N, nsel, npad, host = _common(sy)
    g = sy.grid
    with options(lib, **SINGLE[build]):
        fused, G = int(lib.vmd_hip_cells_fused_ok(g, nsel)), int(lib.vmd_hip_cells_split_blocks(g, nsel))
        assert ("fused" if fused else "split" if G else "atomic") == ROUTE[build], (build, fused, G)
        assert ROUTE[build] != "split" or G == (nsel + SLICE[build] - 1) // SLICE[build]
        words = int(lib.vmd_hip_cells_scratch_words(g, nsel))
        for aos in (False, True):
            buf = Buffers(gpu, cc=np.full(B * (g.ncell + 1), GARBAGE, np.uint32), rank=np.zeros(B * max(words, 1), np.uint32),
                          aos=np.zeros(B * npad * 4, np.float32) if aos else None, **{k: (v.copy() if k in ("cs", "srt") else v) for k, v in host.items()})
            with pattern_of(lib, sy.sel):
                assert lib.vmd_hip_cells_build(None, buf["xyz"], 3 * N, N, buf["g9"], sy.flags, B, buf["sel"], nsel, npad, g,
                                               buf["cc"], buf["rank"], buf["cs"], buf["srt"], buf["aos"]) == 0
            held(sy, O, buf.fetch("cs"), buf.fetch("srt"), f"{build}, aos {aos}, {nsel} atoms, {g.ncell} cells")


COMBOS = tuple((lds, rec3) for lds in (1, 0) for rec3 in (1, 0))            # cells_bin_lds x cells_rec3


def capacities(sy, O, shrink=None):
    """pen_off: per pencil the largest reference population over the frames, rounded up to a multiple of 4"""
    _, cell = sy.reference(O)
    npen = sy.grid.ny * sy.grid.nz
    pop = np.max([np.bincount(c // sy.grid.nxf, minlength=npen) for c in cell], axis=0)
    cap = (pop + 3) & ~3
    if shrink is not None:
        cap[cap > 0] = shrink
    return np.concatenate([[0], np.cumsum(cap)]).astype(np.uint32), int(cap.max()), pop


def pencil(lib, O, sy, lds, rec3, gpu=False, overflow_bit=None):
    """vmd_hip_cells_build_pencil; overflow_bit: the one populated pencil gets a capacity below its population, and only the bit is held"""
    B, N, nsel, npad, host = _common(sy)
    g = sy.grid
    npen = g.ny * g.nz
    pen_off, cap_max, pop = capacities(sy, O, shrink=None if overflow_bit is None else 100)
    total_cap = int(pen_off[npen])
    assert lib.vmd_hip_cells_pencil_ok(g) and 0 < cap_max <= lib.vmd_hip_cells_pencil_cap_max()
    assert overflow_bit is None or ((pop > 0).sum() == 1 and pop.max() > 100)
    buf = Buffers(gpu, pen_off=pen_off, pen_count=np.full(B * npen, GARBAGE, np.uint32), pen_start=np.full(B * (npen + 1), GARBAGE, np.uint32),
                  bucket=np.zeros(B * total_cap * 4, np.float32), overflow=np.zeros(1, np.uint32), **host)
    old_bit = lib.vmd_hip_set_cells_overflow_bit(overflow_bit or 1)
    try:
        with options(lib, cells_bin_lds=lds, cells_rec3=rec3), pattern_of(lib, sy.sel):
            assert lib.vmd_hip_cells_build_pencil(None, buf["xyz"], 3 * N, N, buf["g9"], sy.flags, B, buf["sel"], nsel, npad, g, buf["pen_off"],
                                                  total_cap, cap_max, buf["pen_count"], buf["pen_start"], buf["bucket"], buf["overflow"],
                                                  buf["cs"], buf["srt"]) == 0
    finally:
        lib.vmd_hip_set_cells_overflow_bit(1 if overflow_bit else old_bit)
    if overflow_bit is not None:
        assert int(buf.fetch("overflow")[0]) == overflow_bit
        return
    assert int(buf.fetch("overflow")[0]) == 0
    held(sy, O, buf.fetch("cs"), buf.fetch("srt"), f"two-level, bin_lds {lds}, rec3 {rec3}, {nsel} atoms, {npen} pencils of {g.nxf}")


# ---- the cases --------------------------------------------------------------------------------------------------------------------------

# single-level builds.  nsel: 256-thread blocks (atomic), the 1024-thread stride (fused), 2048- and 1024-atom slices (split)
SINGLE_NSEL = ([("atomic", n) for n in (1, 255, 256, 257)] + [("fused", n) for n in (1, 1023, 1024, 1025)] +
               [("split", n) for n in (2047, 2048, 2049, 4097)] + [("split1024", 1025)])
# ncell: scan chunks of 4096 cells, four per thread (atomic; 24576: both LDS builds refuse it, with and without a switch), stretches of
# ceil(ncell / 1024) cells per thread (fused; 24575 is the last table that fits), rows of 1024 cells (split)
SINGLE_NCELL = ([("atomic", n) for n in (1, 3, 4095, 4096, 4097, 8193, 24576)] + [("default", 24576)] +
                [("fused", n) for n in (1, 1023, 1024, 1025, 2049, 24575)] + [("split", n) for n in (1023, 1024, 1025)])


def single_nsel(lib, O, build, nsel, gpu=False):
    N = nsel + 50
    g = grid3(5, 4, 3)
    single(lib, O, System(1000 + nsel, N, 1, g, sel_list(nsel, nsel, N)), build, gpu)


def single_ncell(lib, O, build, ncell, gpu=False):
    N, nsel = 3300, 3000
    g = grid_of(ncell)
    single(lib, O, System(2000 + ncell, N, 1, g, sel_list(ncell, nsel, N)), build, gpu)


def single_forms(lib, O, build, gpu=False):
    """every form of the index list, three frames; an open x axis"""
    N, g = 2500, grid3(6, 5, 4)
    for i, sel in enumerate(sel_forms(N)):
        single(lib, O, System(3000 + i, N, 3, g, sel), build, gpu)
    single(lib, O, System(3100, N, 3, g, sel_list(3100, 1300, N), flags=6), build, gpu)


# two-level build.  nsel: 4096-atom blocks, four atoms per thread; npen = ny nz: the 256-thread pencil scan and the 1024-thread stretch
# of level 1; nxf: the 256-thread stretch of level 2
PENCIL_NSEL = (1, 1023, 1025, 4095, 4096, 4097, 8193)
PENCIL_NPEN = (1, 255, 256, 257, 1025, 4096)
PENCIL_NXF = (1, 255, 256, 257, 1025)


def pencil_nsel(lib, O, nsel, gpu=False):
    N = nsel + 50
    sy = System(4000 + nsel, N, 1, grid3(5, 4, 4), sel_list(nsel, nsel, N))
    for lds, rec3 in COMBOS:
        pencil(lib, O, sy, lds, rec3, gpu)


def pencil_npen(lib, O, npen, gpu=False):
    N, nsel = 3300, 3000
    sy = System(5000 + npen, N, 1, grid_of_pencils(npen), sel_list(npen, nsel, N))
    for lds, rec3 in COMBOS:
        pencil(lib, O, sy, lds, rec3, gpu)


def pencil_nxf(lib, O, nxf, gpu=False):
    N, nsel = 2200, 2000
    sy = System(6000 + nxf, N, 1, grid3(nxf, 2, 2), sel_list(nxf, nsel, N))
    for lds, rec3 in COMBOS:
        pencil(lib, O, sy, lds, rec3, gpu)


def pencil_forms(lib, O, lds, rec3, gpu=False):
    """every form of the index list, three frames; an open x axis (16-byte records whatever cells_rec3 says), an open z axis"""
    N, g = 2500, grid3(6, 5, 4)
    for i, sel in enumerate(sel_forms(N)):
        pencil(lib, O, System(3000 + i, N, 3, g, sel), lds, rec3, gpu)
    for flags in (6, 3):
        pencil(lib, O, System(3100 + flags, N, 3, g, sel_list(3100, 1300, N), flags=flags), lds, rec3, gpu)


def pencil_overflow(lib, O, lds, rec3, gpu=False):
    """one populated pencil, 300 atoms for a capacity of 100: exactly the thread's bit is raised"""
    N, g = 300, grid3(6, 4, 4)
    sy = System(7000, N, 2, g, Sel(np.arange(N), "absent"), pencil=(1, 2))
    pencil(lib, O, sy, lds, rec3, gpu, overflow_bit=4)
