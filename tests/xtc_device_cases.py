"""The device trajectory decoders (viamd_amd/csrc/vmd_xtc_device.hip: k_xtc_decode, k_xtc_index + k_xtc_chunks, k_xtc_wave plain / with
checkpoints / sectioned, k_xtc_records, k_raw_f32) coordinate by coordinate at the sizes where their launch geometry changes, shared by
tests/test_xtc_device_emu.py (SIMT emulator) and tests/test_xtc_device_gpu.py (MI355X).

Reference: tests/xtc_ref.py alone.  The frames come from xtc_ref.frame_bytes, the expected floats from xtc_ref.to_ints through the contract
of include/vmd_hip.h, fl(fl(int * fl(1/precision)) * 10) in numpy fp32, and everything is compared as bit patterns: no tolerance anywhere.

Every launch goes through guarded_decode: frame_stride is larger than 3 * npad, one more frame's worth of room lies behind the output rows,
the status words, the checkpoint table, the record table and their counters, all of it prefilled with a pattern, and after every launch the
padding columns, the gaps between frames and every trailing guard must still hold the pattern.  A stray store shows on the hardware too,
where no sanitizer watches."""
import functools
import struct

import numpy as np

import xtc_ref

CK_MAX = 64                        # VMD_XTC_CK_MAX (include/vmd_hip.h)
PAT = 0x7fc0dead                   # a quiet NaN with a payload no decoder produces
PAT16 = 0xdead
GAP = 64                           # floats between the frames of the output, words behind every table
BOX = np.diag([60.0, 60.0, 60.0])

# the variants tests/test_xdr.py parametrises, by the same codes: 0 one thread per frame, > 0 index pass + one thread per chunk of that many
# atoms, -1 one wave per frame, -2 wave twice (checkpoints out, then sections from them), -3 / -4 the same on the streams where the file has
# them (4-byte aligned starts), -5 / -6 like -2 / -4 with group records (second pass: k_xtc_records)
VARIANTS = [("thread", 0), ("chunk64", 64), ("chunk300", 300), ("wave", -1), ("wave_ck", -2), ("file_wave", -3), ("file_wave_ck", -4),
            ("wave_rec", -5), ("file_wave_rec", -6)]
TWO_PASS = [(n, c) for n, c in VARIANTS if c in (-2, -4, -5, -6)]
NAMES = {c: n for n, c in VARIANTS}


def ck_tiles_of(natoms):
    """xtc_launch_wave: a checkpoint every ck_tiles-th tile of 64 groups"""
    return max(1, (natoms // 64 + 1 + CK_MAX - 1) // CK_MAX)


def sections_share(B):
    """xtc_launch_wave, mode 2: waves per frame of a sectioned pass"""
    return max(1, min((8192 + B - 1) // B, CK_MAX))


# ---------------------------------------------------------------------------------------------------------------- fixtures
def gas(n, seed):
    """uniform in the 60 A box: almost no runs, one group per atom"""
    return np.random.default_rng(seed).uniform(0.0, 60.0, (3, n)).astype(np.float32)


def water(n, seed):
    """rigid three-site molecules on a jittered lattice, cut after n atoms: runs of 2, few groups per atom"""
    rng = np.random.default_rng(seed)
    m = (n + 2) // 3
    side = int(np.ceil(m ** (1.0 / 3.0)))
    o = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 3)[:m] * 3.1
    o = o + rng.uniform(-0.3, 0.3, o.shape) + 1.0
    u = rng.normal(0, 1, (m, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(u, rng.normal(0, 1, (m, 3))); v /= np.linalg.norm(v, axis=1, keepdims=True)
    half = np.radians(104.52 / 2)
    h = o[:, None, :] + 0.9572 * np.stack([np.cos(half) * u + np.sin(half) * v, np.cos(half) * u - np.sin(half) * v], axis=1)
    w = np.concatenate([o[:, None, :], h], axis=1).reshape(-1, 3)[:n]
    return w.T.astype(np.float32)


def ten(n, seed):
    assert n == 10
    return np.random.default_rng(seed).uniform(0.0, 10.0, (3, 10)).astype(np.float32)


FIXTURES = {"gas": gas, "water": water, "ten": ten}
SHIFT = np.array([0.37, 1.13, -0.71], np.float32)      # frame k of a batch is moved by k * SHIFT: its own minint, maxint (and smallidx)


@functools.lru_cache(maxsize=None)
def encoded(kind, n, seed, k, precision):
    """-> (frame bytes, expected floats [3, n] as uint32 bit patterns, atom groups in the stream); computed once per process"""
    xyz = FIXTURES[kind](n, seed) + (SHIFT * np.float32(k))[:, None]
    frame = xtc_ref.frame_bytes(xyz, BOX, k, 0.0, precision)
    ints = xtc_ref.to_ints((xyz * np.float32(0.1)).T, precision)
    st = {}
    xtc_ref.compress(ints, st)
    invp = np.float32(1.0) / np.float32(precision)
    want = np.ascontiguousarray(((ints.astype(np.float32) * invp) * np.float32(10.0)).T)
    want.flags.writeable = False
    return frame, want.view(np.uint32), st["flag0"] + st["flag1"]


def expected_checkpoints(natoms, groups):
    """a first pass drops one at the start of every ck_tiles-th tile of 64 groups"""
    tiles = (groups + 63) // 64
    t = ck_tiles_of(natoms)
    return (tiles + t - 1) // t


# ---------------------------------------------------------------------------------------------------------------- memory
class Mem:
    """an array the kernels see: device memory from torch on the GPU (hipMalloc: 256-byte aligned), 64-byte aligned host memory for the
    emulator build, where "device" memory is host memory"""

    def __init__(self, host, gpu):
        host = np.ascontiguousarray(host)
        self.dtype, self.shape, self.gpu = host.dtype, host.shape, gpu
        flat = host.reshape(-1).view(np.uint8)
        if gpu:
            import torch
            self.t = torch.from_numpy(flat.copy()).cuda()
            self.ptr = self.t.data_ptr()
        else:
            self.store = np.zeros(flat.size + 64, np.uint8)
            base = (-self.store.ctypes.data) % 64
            self.a = self.store[base:base + flat.size]
            self.a[:] = flat
            self.ptr = self.a.ctypes.data

    def get(self):
        b = self.t.cpu().numpy() if self.gpu else self.a.copy()
        return b.view(self.dtype).reshape(self.shape)

    def put(self, host):
        flat = np.ascontiguousarray(host).reshape(-1).view(np.uint8)
        if self.gpu:
            import torch
            self.t.copy_(torch.from_numpy(flat.copy()))
        else:
            self.a[:] = flat


def _sync(gpu):
    if gpu:
        import torch
        torch.cuda.synchronize()


class Decoded:
    def __init__(self):
        self.out = self.first = self.status = self.nck = self.nrec = None


def _filled(n, value, dtype=np.uint32):
    return np.full(n, value, dtype)


def guarded_decode(lib, blob, natoms, chunk=0, gpu=False, prefix=8, both_phases=True, groups=None):
    """Run one variant (the codes of VARIANTS) on every frame of an XTC byte string, inside guards.  Returns what the decoder left: out
    [B, 3, natoms] fp32 (the second pass of a two-pass variant; .first is the first pass), the status words, the checkpoint and record
    counts.  `groups` (per frame, from the reference encoder) additionally pins the counts a clean first pass must report."""
    import ctypes as C
    from viamd_amd import _lib as L
    with_rec = chunk in (-5, -6)
    if with_rec:
        chunk = -2 if chunk == -5 else -4
    file_layout = chunk in (-3, -4)
    if file_layout:
        chunk += 2
    off, infos, streams, starts = 0, [], [], []
    while off < len(blob):
        n = struct.unpack_from(">i", blob, off + 4)[0]
        precision, = struct.unpack_from(">f", blob, off + 56)
        mm = struct.unpack_from(">7i", blob, off + 60)
        nbytes, = struct.unpack_from(">i", blob, off + 88)
        streams.append(blob[off + 92: off + 92 + nbytes])
        starts.append(off + 92)
        infos.append((precision, mm[0:3], mm[3:6], mm[6], nbytes))
        off += 92 + ((nbytes + 3) & ~3)
        assert n == natoms
    B = len(infos)
    raw = bytearray()
    arr = (L.XtcFrame * B)()
    for b, (precision, mi, ma, sidx, nbytes) in enumerate(infos):
        arr[b].precision = precision
        arr[b].minint[:] = mi
        arr[b].maxint[:] = ma
        arr[b].smallidx = sidx
        arr[b].offset = prefix + starts[b] if file_layout else len(raw)
        arr[b].nbytes = nbytes
        if not file_layout:
            raw += streams[b] + b"\0" * ((-len(streams[b])) % 64 + 64)
    if file_layout:
        # what the evaluator DMAs out of the mapped file: 4-byte aligned starts, the next frame's header as the readable bytes behind a stream
        assert prefix >= 8 and prefix % 4 == 0
        raw = bytearray(b"\xa5" * prefix + blob + b"\xa5" * 64)
        if both_phases:
            assert len({int(a.offset) % 8 for a in arr}) == 2 or B < 4, "fixture without both phases"
    npad = (natoms + 63) & ~63
    frame_stride = 3 * npad + GAP
    d_raw = Mem(np.frombuffer(bytes(raw), np.uint8), gpu)
    d_info = Mem(np.frombuffer(bytes(arr), np.uint8), gpu)
    fresh_out = _filled((B + 1) * frame_stride, PAT).reshape(B + 1, frame_stride)
    d_out = Mem(fresh_out, gpu)
    d_status = Mem(np.concatenate([_filled(B, 99), _filled(GAP, PAT)]), gpu)
    raw_p, info_p, out_p, status_p = d_raw.ptr, d_info.ptr, d_out.ptr, d_status.ptr
    r = Decoded()

    def check_out(what):
        """-> the frames' floats; the padding columns, the gaps between the frames and the frame behind the last are untouched"""
        o = d_out.get()
        rows = o[:B, :3 * npad].reshape(B, 3, npad)
        assert (rows[:, :, natoms:] == PAT).all(), f"{what}: a store into the padding columns [{natoms}, {npad})"
        assert (o[:B, 3 * npad:] == PAT).all(), f"{what}: a store between two frames"
        assert (o[B] == PAT).all(), f"{what}: a store behind the last frame"
        st = d_status.get()
        assert (st[B:] == PAT).all(), f"{what}: a store behind the status words"
        return np.ascontiguousarray(rows[:, :, :natoms]).view(np.float32), st[:B].copy()

    if chunk == -2:
        rec_stride = npad + GAP
        d_ck = Mem(_filled((B + 1) * CK_MAX * 4, PAT).reshape(B + 1, CK_MAX, 4), gpu)
        d_nck = Mem(np.concatenate([np.zeros(B, np.uint32), _filled(GAP, PAT)]), gpu)
        if with_rec:
            d_rec = Mem(_filled((B + 1) * rec_stride, PAT16, np.uint16).reshape(B + 1, rec_stride), gpu)
            d_nrec = Mem(np.concatenate([np.zeros(B, np.uint32), _filled(GAP, PAT)]), gpu)
            two_pass = lambda use: lib.vmd_hip_xtc_decode_wave_rec(None, raw_p, info_p, B, natoms, out_p, frame_stride, npad, status_p, use,
                                                                   d_ck.ptr, d_nck.ptr, d_rec.ptr, d_nrec.ptr, rec_stride)
        else:
            two_pass = lambda use: lib.vmd_hip_xtc_decode_wave_ck(None, raw_p, info_p, B, natoms, out_p, frame_stride, npad, status_p, use,
                                                                  d_ck.ptr, d_nck.ptr)

        def check_tables(what, clean):
            ck, nck = d_ck.get(), d_nck.get()
            assert (ck[B] == PAT).all(), f"{what}: a store behind the checkpoint table"
            assert (nck[B:] == PAT).all(), f"{what}: a store behind the checkpoint counters"
            rec = nrec = None
            if with_rec:
                rec, nrec = d_rec.get(), d_nrec.get()
                assert (rec[B] == PAT16).all(), f"{what}: a store behind the record table"
                assert (nrec[B:] == PAT).all(), f"{what}: a store behind the record counters"
            if clean:
                counts = nck[:B]
                assert (counts >= 1).all() and (counts <= CK_MAX).all(), counts
                for f in range(B):
                    c = int(counts[f])
                    assert (ck[f, c:] == PAT).all(), f"{what}: frame {f} reports {c} checkpoints and wrote more"
                    assert tuple(ck[f, 0]) == (0, 0, infos[f][3], 0), (what, f, ck[f, 0])        # the stream's first bit, the header's smallidx
                    assert (ck[f, :c, 3] == 0).all() and (np.diff(ck[f, :c, 1].astype(np.int64)) > 0).all() and ck[f, c - 1, 1] < natoms
                if groups is not None:
                    np.testing.assert_array_equal(counts, [expected_checkpoints(natoms, g) for g in groups], err_msg=what)
                if with_rec:
                    ng = nrec[:B]
                    assert (ng >= 1).all() and (ng <= natoms).all(), ng                        # every frame got its records: one per group
                    for f in range(B):
                        assert (rec[f, int(ng[f]):] == PAT16).all(), f"{what}: frame {f} reports {ng[f]} records and wrote more"
                    if groups is not None:
                        np.testing.assert_array_equal(ng, groups, err_msg=what)
            return ck, nck, rec, nrec

        rc = two_pass(0)
        assert rc == 0
        _sync(gpu)
        first, st1 = check_out("first pass")
        clean = bool((st1 == 0).all())
        tables = check_tables("first pass", clean)
        r.first, r.out, r.status = first, first, st1
        r.nck = tables[1][:B].copy()
        r.nrec = tables[3][:B].copy() if with_rec else None
        if clean:
            d_out.put(fresh_out)
            rc = two_pass(1)
            _sync(gpu)
            second, st2 = check_out("second pass")
            again = check_tables("second pass", True)
            for a, b in zip(tables, again):                                                   # a second pass reads the tables, nothing else
                if a is not None:
                    np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(second.view(np.uint32), first.view(np.uint32))      # sections == one walk, bit for bit
            r.out, r.status = second, st2
    else:
        if chunk == -1:          # one wave per frame (k_xtc_wave)
            rc = lib.vmd_hip_xtc_decode_wave(None, raw_p, info_p, B, natoms, out_p, frame_stride, npad, status_p)
        elif chunk:              # two passes: index (one thread per frame) + chunks (one thread per chunk)
            words = lib.vmd_hip_xtc_scratch_bytes(B, natoms, chunk) // 8 + 1
            d_scratch = Mem(np.concatenate([np.zeros(words, np.uint64), _filled(2 * GAP, PAT, np.uint64)]), gpu)
            rc = lib.vmd_hip_xtc_decode_chunked(None, raw_p, info_p, B, natoms, out_p, frame_stride, npad, status_p, chunk, d_scratch.ptr)
        else:
            rc = lib.vmd_hip_xtc_decode(None, raw_p, info_p, B, natoms, out_p, frame_stride, npad, status_p)
        _sync(gpu)
        r.out, r.status = check_out("decode")
        if chunk > 0:
            assert (d_scratch.get()[words:] == PAT).all(), "a store behind the scratch block of the chunked decode"
    assert rc == 0, f"launch of the device decoder (chunk {chunk}) returned {rc}"
    return r


# ---------------------------------------------------------------------------------------------------------------- cases
def run_case(lib, label, kind, n, seeds, B, precision, chunk, gpu, tmp_path=None, prefixes=(8, 12)):
    """A batch of B frames that repeats len(seeds) distinct encoded frames cyclically (frame k: fixture of seeds[k], moved by k * SHIFT)
    through one variant: status 0, every coordinate of every pass bit-identical to the reference, guards intact.  The file-layout variants
    run with the file at both 4-byte phases, so every stream is entered at 0 and at 4 modulo 8."""
    k = len(seeds)
    enc = [encoded(kind, n, seeds[j], j, float(precision)) for j in range(k)]
    blob = b"".join(enc[b % k][0] for b in range(B))
    want = np.stack([enc[b % k][1] for b in range(B)])
    groups = [enc[b % k][2] for b in range(B)]
    r = None
    for prefix in (prefixes if chunk in (-3, -4, -6) else (8,)):
        r = guarded_decode(lib, blob, n, chunk, gpu, prefix=prefix, both_phases=False, groups=groups)
        assert (r.status == 0).all(), (label, chunk, r.status)
        np.testing.assert_array_equal(r.out.view(np.uint32), want, err_msg=f"{label}, variant {chunk}, prefix {prefix}")
        if r.first is not None:
            np.testing.assert_array_equal(r.first.view(np.uint32), want, err_msg=f"{label}, variant {chunk}, prefix {prefix}: first pass")
    if tmp_path is not None:
        # the file is written anyway: the host reader returns the same floats
        import viamd_amd as V
        p = tmp_path / "case.xtc"
        p.write_bytes(blob)
        t = V.XdrTrajectory(p, lib=lib)
        assert (t.num_frames(), t.num_atoms()) == (B, n)
        for b in sorted({0, min(1, B - 1), min(2, B - 1), B - 1}):
            np.testing.assert_array_equal(t.load_frame(b)[0].view(np.uint32), want[b], err_msg=f"{label}: load_frame({b})")
        t.close()
    ck = "" if r.nck is None else f", checkpoints {int(r.nck.min())}..{int(r.nck.max())}"
    print(f"xtc_device {label}: variant {NAMES[chunk]} ({chunk}), B = {B}, natoms = {n}, precision {precision:g}, groups {min(groups)}..{max(groups)}{ck}: "
          f"{want.size} coordinates bit-identical, guards intact")
    return r


# seeds searched with the reference encoder and confirmed on the emulator: every frame of the 4 095- and 8 191-atom fixtures has more than
# 63 (x ck_tiles) full tiles of groups and so leaves exactly VMD_XTC_CK_MAX checkpoints (a gas still has runs, the count depends on the seed)
GAS_SEEDS = {4031: (1, 2), 4032: (1, 2), 4095: (1, 4, 5), 4096: (1, 2), 4097: (1, 2), 8191: (1, 2), 8192: (1, 2)}
EXACTLY_64 = (4095, 8191)
ATOM_EDGES = [("gas", n) for n in sorted(GAS_SEEDS)] + [("water", 4096), ("water", 8192)]


def atom_count_edge(lib, kind, n, chunk, gpu, tmp_path=None):
    """4 031 .. 8 192 atoms, two frames: ck_tiles 1, 2 and 3, the last tile full / one short / one over, and - for the pinned gas frames of
    4 095 and 8 191 atoms - the last slot of a frame's row of the checkpoint table"""
    seeds = GAS_SEEDS[n][:2] if kind == "gas" else (5, 6)
    assert ck_tiles_of(n) == (1 if n < 4096 else 2 if n < 8192 else 3)
    r = run_case(lib, f"{kind} {n}", kind, n, seeds, 2, 1000.0, chunk, gpu, tmp_path)
    if r.nck is not None:
        assert (r.nck >= 1).all() and (r.nck <= CK_MAX).all(), r.nck
        if kind == "gas" and n in EXACTLY_64:
            assert (r.nck == CK_MAX).all(), f"the pinned {n}-atom gas frames no longer leave exactly {CK_MAX} checkpoints: {r.nck}"
    return r


def chunked_past_64_chunks(lib, gpu):
    """k_xtc_chunks launches (maxck + 63) / 64 blocks of 64 chunk threads: a second x-block needs more than 64 chunks in a frame"""
    n, chunk = 4097, 64
    maxck = (n + chunk - 1) // chunk + 1                          # vmd_hip_xtc_decode_chunked
    assert maxck > 64
    run_case(lib, f"gas {n}, {maxck} chunk slots", "gas", n, GAS_SEEDS[n], 2, 1000.0, chunk, gpu)
    run_case(lib, f"water 8192, {(8192 + chunk - 1) // chunk + 1} chunk slots", "water", 8192, (5, 6), 2, 1000.0, chunk, gpu)


B_EDGES = [("ten", 10, 64), ("ten", 10, 65), ("ten", 10, 130), ("water", 640, 70)]


def batch_edge(lib, kind, n, B, chunk, gpu):
    """B > 64: the second (and third) block of the frame-per-thread kernels; for the sectioned passes share = ceil(8192 / B) drops to 1
    with the smallest compressed frame"""
    return run_case(lib, f"{kind} {n} x {B}", kind, n, (7, 8, 9), B, 1000.0, chunk, gpu)


def fewer_waves_than_sections(lib, chunk, gpu, prefixes=(8, 12)):
    """B = 160 frames of exactly 64 checkpoints: the sectioned passes get 52 waves for 64 sections, so a wave owns more than one"""
    B, n = 160, 4095
    r = run_case(lib, f"gas {n} x {B}", "gas", n, GAS_SEEDS[n], B, 1000.0, chunk, gpu, prefixes=prefixes)
    share = sections_share(B)
    assert (r.nck == CK_MAX).all(), r.nck
    assert share < int(r.nck.min()), (share, r.nck.min())
    return r


PRECISIONS = [("gas", 8192, 100.0), ("gas", 8192, 12345.0), ("water", 640, 100.0), ("water", 640, 12345.0)]


def precision_case(lib, kind, n, precision, chunk, gpu):
    """100: the large triple of the 60 A box fits 32 bits (the short path of xtc_triple); 12345: a 49-bit number, 1 / precision inexact"""
    seeds = GAS_SEEDS[n] if kind == "gas" else (7, 8)
    return run_case(lib, f"{kind} {n} precision {precision:g}", kind, n, seeds, 2, precision, chunk, gpu)


# ---------------------------------------------------------------------------------------------------------------- every atom, evaluator
def add_every_atom(ir, N, name="every_atom"):
    """distance_pair(four anchor atoms, every atom): each atom's coordinates determine its own four distances (the anchors of a liquid are
    never collinear), so one wrong hydrogen - or a wrong last atom - changes the rows, where an O-O histogram never sees two thirds of
    the atoms"""
    from viamd_amd import _lib as L
    anchors = np.array([0, N // 3 + 1, (2 * N) // 3 + 2, N - 1], np.int32)
    assert len(set(anchors.tolist())) == 4
    ir.add_distance(name, anchors, np.arange(N, dtype=np.int32), L.DIST_PAIR)


def every_atom_rows(ev, N, name="every_atom"):
    """-> [frames, 4 * N] as bit patterns"""
    pd = ev.property_data(name)
    rows = np.ascontiguousarray(pd.values, np.float32).reshape(pd.dim[0], -1).copy().view(np.uint32)
    assert rows.shape[1] == 4 * N, rows.shape
    return rows


# ---------------------------------------------------------------------------------------------------------------- k_raw_f32
F32_SHAPES = [1, 255, 256, 257, 1000]


def raw_f32_case(lib, natoms, gpu, B=3):
    """vmd_hip_raw_f32_decode on byte strings built in numpy: planar (a block per component with 8-byte gaps, as DCD has) and interleaved
    (xyz per atom, as TRR has), either byte order, scale 1 (no multiply) and 10, every frame on a 4-byte but not 8-byte boundary.  Expected:
    the numpy fp32 product (the input itself for scale 1) as uint32 bit patterns - denormals, -0.0 and a value near 3e37 included, which is
    what the host readers (vmd_xdr.cpp trr_load, vmd_dcd.cpp) return."""
    from viamd_amd import _lib as L
    rng = np.random.default_rng(100 + natoms)
    npad = (natoms + 63) & ~63
    frame_stride = 3 * npad + GAP
    vals = (rng.normal(0.0, 30.0, (B, 3, natoms)) * 10.0 ** rng.integers(-3, 3, (B, 3, natoms))).astype(np.float32)
    special = np.array([1e-40, -0.0, 3e37], np.float32)
    for b in range(B):
        for c in range(3):                                          # one of the three per component, rotating with the frame
            vals[b, c, [0, natoms // 2, natoms - 1][c]] = special[(b + c) % 3]
    assert np.isfinite(vals).all() and (np.abs(vals[vals != 0]) < 1.2e-38).any() and np.signbit(vals[vals == 0]).any()
    for layout in ("planar", "interleaved"):
        for big in (0, 1):
            for scale in (1.0, 10.0):
                raw = bytearray(b"\xa5" * 4)
                info = (L.F32Frame * B)()
                dt = ">f4" if big else "<f4"
                for b in range(B):
                    # the frame's first float lies at 4 modulo 8 (planar: behind its 4-byte record marker)
                    raw += b"\xa5" * (((0 if layout == "planar" else 4) - len(raw)) % 8)
                    if layout == "planar":
                        for c in range(3):
                            raw += b"\x5a" * 4                      # the record marker in front of a block, ...
                            info[b].offset[c] = len(raw)
                            raw += vals[b, c].astype(dt).tobytes()
                            raw += b"\x5a" * 4                      # ... and behind it: 8 bytes between two planes
                        info[b].stride = 1
                    else:
                        for c in range(3):
                            info[b].offset[c] = len(raw) + 4 * c
                        raw += np.ascontiguousarray(vals[b].T).astype(dt).tobytes()
                        info[b].stride = 3
                    info[b].flags = big
                    info[b].scale = scale
                    info[b].reserved = 0
                    assert all(int(o) % 4 == 0 for o in info[b].offset) and int(info[b].offset[0]) % 8 == 4
                raw += b"\xa5" * 64
                d_raw = Mem(np.frombuffer(bytes(raw), np.uint8), gpu)
                d_info = Mem(np.frombuffer(bytes(info), np.uint8), gpu)
                d_out = Mem(_filled((B + 1) * frame_stride, PAT).reshape(B + 1, frame_stride), gpu)
                rc = lib.vmd_hip_raw_f32_decode(None, d_raw.ptr, d_info.ptr, B, natoms, d_out.ptr, frame_stride, npad)
                _sync(gpu)
                assert rc == 0
                o = d_out.get()
                rows = o[:B, :3 * npad].reshape(B, 3, npad)
                what = f"raw_f32 natoms {natoms} {layout} {'big' if big else 'little'}-endian scale {scale:g}"
                assert (rows[:, :, natoms:] == PAT).all(), f"{what}: a store into the padding columns"
                assert (o[:B, 3 * npad:] == PAT).all(), f"{what}: a store between two frames"
                assert (o[B] == PAT).all(), f"{what}: a store behind the last frame"
                want = vals if scale == 1.0 else vals * np.float32(scale)
                assert want.dtype == np.float32
                np.testing.assert_array_equal(rows[:, :, :natoms], want.view(np.uint32), err_msg=what)
                print(f"xtc_device {what}: {want.size} floats bit-identical, guards intact")
