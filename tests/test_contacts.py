"""Residue contact maps and the native-contact fraction on the emulator build and in the host-only entry points.  The rule is
EXACT EQUALITY with the numpy restatement (tests/contact_ref.py) for every output - the counts per frame, every accumulator of the record,
the Q floats, the pair lists of a frame - and every launch choice (walk or all pairs, batch size, call pattern) bit-identical to the
others.  Every check prints how many candidate entry pairs lie within 4 ulp of r_cut, so that a reader sees the equality was exercised; a
closing test asserts that the threshold scenarios did produce such pairs.  Scenarios: known answers (two one-atom groups across the faces,
an edge and a corner of a cell, tilted and with an open axis; a four-residue chain under min_sep 1, 2, 3); the size edges of the list and
of the pair index, in three cells, by every route; 2048 groups; duplicates; planted thresholds under both spec_within_closed settings;
small boxes; identity and coincidence; Q; the call patterns; a batch repeated for a bucket overflow; the two-rank merge; and the host-only
part - every refusal, the fingerprint field by field, the topology helper, the statement next to the default script and the other forms.
tests/test_contacts_gpu.py runs the same scenario functions on the device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import viamd_amd as V
from viamd_amd import _lib as L
from viamd_amd import script

import cases
import contact_cases as CC
import contact_ref as R
import hbond_cases as HC
import sasa_cases as SC
import ss_cases as SS
import test_geometry as TG
import test_rmsd as TR
from test_hbond import Options, ref_box, steps
from test_rama import OPT_INS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nc", "cmap")
QNAME = "q"
WALK, BRUTE = dict(shell_brute_below=0), dict(shell_brute_below=1 << 30)
ROUTES = (dict(), WALK, BRUTE)
NEAR = {}                        # what -> candidate entry pairs within 4 ulp of r_cut, as printed
ROOMY = ((30.0, 30.0, 30.0), (0.0, 0.0, 0.0), 7)


def ct_ir(lib, sites, r=CC.R_CUT, min_sep=CC.MIN_SEP, native=None, names=NAMES):
    ir = V.ScriptIR(lib)
    have = native is not None and len(native) > 0
    ir.add_contacts(tuple(names) + ((QNAME,) if have else ()), sites["atoms"], sites["groups"], r, min_sep, native=native,
                    ngroups=sites["ngroups"])
    return ir


class Run:
    """one evaluation: the eval and what a single-frame query needs"""

    def __init__(self, lib, ir, coords, cell, device=False, ranges=None, pooled=None):
        box, tilt, flags = cell
        F, _, N = coords.shape
        self.cell = V.make_unitcell(box, flags, tilt)
        self.ev = V.ScriptEval(F, ir)
        self.sysm = V.MolSystem(N, unitcell=self.cell)
        self.traj = cases.make_traj(lib, coords, self.cell, device)
        for beg, end in ([(0, F)] if ranges is None else ranges):
            assert (self.ev.frame_range_pooled(self.sysm, self.traj, beg, end, *pooled) if pooled else
                    self.ev.frame_range(self.sysm, self.traj, beg, end))

    def counts(self, name=NAMES[0]):
        return TG.rows(self.ev, name)[:, 0]

    def q(self):
        return TG.rows(self.ev, QNAME)[:, 0] if QNAME in self.ev.ir.property_names() else np.zeros(0, np.float32)

    def record(self, name=NAMES[1]):
        return self.ev.property_data(name).contact_accumulators.copy()

    def pairs(self, frame, name=NAMES[0]):
        return self.ev.contact_pairs(name, self.sysm, self.traj, frame)

    def out(self):
        return self.counts(), self.record(), self.q()


def run(lib, sites, coords, cell, device=False, r=CC.R_CUT, min_sep=CC.MIN_SEP, native=None, **kw):
    return Run(lib, ct_ir(lib, sites, r, min_sep, native), coords, cell, device, **kw)


def restate(coords, cell, sites, r=CC.R_CUT, min_sep=CC.MIN_SEP, native=None, closed=False, frames=None):
    bx, flags = ref_box(cell)
    return R.evaluate(coords, bx, sites["atoms"], sites["groups"], sites["ngroups"], r, min_sep, native=native, closed=closed, flags=flags,
                      frames=frames)


def check(rn, want, sites, what, list_frames=None):
    """every output against the restatement `want`, exactly, and the invariants of every scenario"""
    G = sites["ngroups"]
    P = G * (G - 1) // 2
    got_c, got_r, got_q = rn.out()
    NEAR[what] = want["near"]
    frames = sorted(want["pairs"])
    print(f"{what}: {int(want['record'][:-1].sum())} contacts in {int(want['record'][-1])} frames, {want['near']} candidate entry pairs "
          f"within 4 ulp of r_cut")
    assert got_c.dtype == np.float32 and np.array_equal(got_c.view(np.int32), want["counts"].view(np.int32)), what
    assert got_r.dtype == np.uint64 and got_r.shape == (P + 1,) and np.array_equal(got_r, want["record"]), what
    if want["q"] is not None:
        assert got_q.dtype == np.float32 and np.array_equal(got_q.view(np.int32), want["q"].view(np.int32)), what
    # invariants: a row never exceeds the frames; without a frame twice the rows add up to the counts
    assert (got_r[:-1] <= got_r[-1]).all(), what
    if int(got_r[-1]) == len(frames):
        assert int(got_r[:-1].sum()) == int(got_c[frames].sum()), what
    # the reader, under every name of the statement, condensed and square
    occ, F = rn.ev.contacts(NAMES[1])
    assert F == int(got_r[-1]) and np.array_equal(occ, got_r[:-1] / max(F, 1)), what
    if G <= 65:
        sq, _ = rn.ev.contacts(NAMES[0], square=True)
        assert sq.shape == (G, G) and np.array_equal(sq, sq.T) and not np.diag(sq).any() and np.array_equal(sq[np.triu_indices(G, 1)], occ), what
    for f in (frames if list_frames is None else list_frames):
        got = rn.pairs(f)
        assert got.dtype == np.int32 and got.shape == want["pairs"][f].shape and np.array_equal(got, want["pairs"][f]), (what, f)
        assert len(got) == int(want["counts"][f]), (what, f)
    return got_c, got_r, got_q


def same(a, b, what):
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[2].view(np.int32), b[2].view(np.int32)), what


def all_routes(lib, sites, coords, cell, want, what, device=False, list_frames=None, r=CC.R_CUT, min_sep=CC.MIN_SEP, native=None, **opts):
    one = None
    for route in ROUTES:
        with Options(lib, **dict(opts, **route)):
            got = check(run(lib, sites, coords, cell, device, r, min_sep, native), want, sites, f"{what}, {route}", list_frames)
        one = one or got
        same(got, one, (what, route))
    return one


def one_per_group(n):
    return dict(atoms=np.arange(n, dtype=np.int32), groups=np.arange(n, dtype=np.int32), ngroups=n)


# ---- 1. known answers -------------------------------------------------------------------------------------------------------------------------

def known_answers(lib, device=False):
    """Two groups of one atom each, 3 A apart: frame by frame the pair is moved so that it crosses each face, an edge and a corner of a
    cubic cell; the same in a tilted cell; with the x axis open the pair across the x face is no pair.  One bit, P = 1."""
    rng = np.random.default_rng(2)
    L_ = 20.0
    spots = [(10.0, 10.0, 10.0), (L_ - 1.0, 10.0, 10.0), (10.0, L_ - 1.0, 10.0), (10.0, 10.0, L_ - 1.0), (L_ - 1.0, L_ - 0.5, 10.0),
             (L_ - 0.5, L_ - 0.5, L_ - 0.5), (-1.0, 3.0 * L_ + 0.5, -L_ - 1.0)]
    axes = [np.eye(3), np.eye(3), np.eye(3)[[1, 0, 2]], np.eye(3)[[2, 1, 0]]]
    frames = []
    for k, sp in enumerate(spots):
        rot = axes[k] if k < 4 else HC.rotation(rng)
        frames.append((np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]]) @ rot.T + np.asarray(sp)).T)
    coords = np.stack(frames).astype(np.float32)
    sites = one_per_group(2)
    for cell in (((L_, L_, L_), (0.0, 0.0, 0.0), 7), ((L_, L_, L_), (4.0, -2.0, 3.0), 7)):
        want = restate(coords, cell, sites, min_sep=1)
        assert list(want["counts"]) == [1.0] * len(spots) and list(want["record"]) == [len(spots)] * 2
        got = all_routes(lib, sites, coords, cell, want, f"one pair, tilt {cell[1]}", device, min_sep=1)
        assert list(got[1]) == [len(spots), len(spots)]
    folded = coords.copy()
    folded[:6] = np.mod(folded[:6], np.float32(L_))
    cell = ((L_, L_, L_), (0.0, 0.0, 0.0), 6)
    want = restate(folded, cell, sites, min_sep=1)
    assert list(want["counts"][:4]) == [1.0, 0.0, 1.0, 1.0]                # across the open x face: no pair (edge and corner: as they turn out)
    all_routes(lib, sites, folded, cell, want, "one pair, x open", device, min_sep=1)
    # a four-residue chain: residue 1 far away, residues 2 and 3 each 4 A from residue 0 and 5.7 A from each other
    chain4 = np.array([[[5.0, 20.0, 9.0, 5.0], [5.0, 20.0, 5.0, 9.0], [5.0, 20.0, 5.0, 5.0]]], np.float32)
    sites = one_per_group(4)
    for ms, pairs in ((1, [(0, 2), (0, 3)]), (2, [(0, 2), (0, 3)]), (3, [(0, 3)])):
        want = restate(chain4, ROOMY, sites, min_sep=ms)
        assert [tuple(p) for p in want["pairs"][0]] == pairs
        got = all_routes(lib, sites, chain4, ROOMY, want, f"four residues, min_sep {ms}", device, min_sep=ms)
        assert list(np.nonzero(got[1][:-1])[0]) == [int(R.pair_index(4, g, h)) for g, h in pairs]


def test_known_answers_on_the_emulator(emu_lib):
    known_answers(emu_lib)


# ---- 2. size edges ----------------------------------------------------------------------------------------------------------------------------

def size_sweep(lib, ci, device=False):
    """(entries, groups) of contact_cases in cell ci: the default route (all pairs below 480 entries, the walk from there), the walk and
    all pairs forced through shell_brute_below, each with batch_frames 1 and 2 - one answer"""
    cell = CC.CELLS[ci]
    for n, G in CC.SIZES:
        coords = CC.chain(n, cell[0], 2, seed=3 + ci)
        sites = CC.sites(n, G)
        ms = CC.min_sep_of(G)
        want = restate(coords, cell, sites, min_sep=ms)
        what = f"cell {ci}, {n} entries in {G} groups"
        assert n < 63 or want["record"][:-1].any(), what
        one = None
        for route in ROUTES:
            for bf in (1, 2):
                with Options(lib, batch_frames=bf, **route):
                    rn = run(lib, sites, coords, cell, device, min_sep=ms)
                    if one is None:
                        one = check(rn, want, sites, what, list_frames=[1])
                    else:
                        same(rn.out(), one, (what, route, bf))
        if device and n == 481:
            same(run(lib, sites, coords, cell, min_sep=ms).out(), one, (what, "host-staged"))


@pytest.mark.parametrize("ci", range(len(CC.CELLS)))
def test_size_edges_on_the_emulator(emu_lib, ci):
    size_sweep(emu_lib, ci)


def largest_index(lib, device=False):
    """2048 groups, 300 entries, two frames: the pair index at its largest (P = 2 096 128 = 65 504 words exactly; the size sweep has the
    partly used last words); entries in the first and the last groups"""
    G, n = 2048, 300
    coords = CC.chain(n, ROOMY[0], 2, seed=41, step=2.0)
    groups = np.sort(np.concatenate([[0, 1, 2, G - 3, G - 2, G - 1], np.random.default_rng(5).integers(0, G, n - 6)])).astype(np.int32)
    # the chain's ends meet: the first and the last entries (groups 0 and 2047) on neighbouring points
    coords = coords.copy()
    coords[:, :, n - 1] = coords[:, :, 0] + np.float32(1.5)
    sites = dict(atoms=np.arange(n, dtype=np.int32), groups=groups, ngroups=G)
    want = restate(coords, ROOMY, sites)
    P = G * (G - 1) // 2
    assert want["record"][R.pair_index(G, 0, G - 1)] == 2 and R.pair_index(G, G - 2, G - 1) == P - 1
    all_routes(lib, sites, coords, ROOMY, want, "2048 groups", device, list_frames=[1])
    with pytest.raises(V.VmdError, match=r"\[2, 2048\]"):
        ct_ir(lib, dict(sites, ngroups=G + 1))


def test_largest_index_on_the_emulator(emu_lib):
    largest_index(emu_lib)


def duplicates(lib, device=False):
    """two groups of ten atoms, every one of the 100 atom pairs within r_cut: the pair counts once per frame"""
    rng = np.random.default_rng(7)
    F = 3
    a = np.array([5.0, 5.0, 5.0]) + rng.uniform(-0.5, 0.5, (F, 10, 3))
    b = np.array([7.5, 5.0, 5.0]) + rng.uniform(-0.5, 0.5, (F, 10, 3))
    coords = np.concatenate([a, b], axis=1).transpose(0, 2, 1).astype(np.float32)
    assert np.linalg.norm(a[:, :, None] - b[:, None, :], axis=-1).max() < CC.R_CUT
    sites = dict(atoms=np.arange(20, dtype=np.int32), groups=np.repeat([0, 1], 10).astype(np.int32), ngroups=2)
    want = restate(coords, ROOMY, sites, min_sep=1)
    assert list(want["record"]) == [F, F] and list(want["counts"]) == [1.0] * F
    all_routes(lib, sites, coords, ROOMY, want, "100 atom pairs behind one bit", device, min_sep=1)


def test_duplicates_on_the_emulator(emu_lib):
    duplicates(emu_lib)


def lds_rows(lib, device=False):
    """option contact_lds_rows: the walk that ORs a block's hits into LDS bit rows first against the direct one - contiguous groups (a
    block's rows fit), more than one block, a last block with idle lanes, scattered groups and 2048 groups (a block's run of rows does
    not fit: the direct path inside the variant), coincident entries - one answer, the restatement's"""
    cell = CC.CELLS[1]
    cases_ = []
    for n, G in ((65, 65), (257, 64), (481, 64), (700, 70)):
        cases_.append((f"{n} entries in {G} groups", CC.chain(n, cell[0], 2, seed=31), CC.sites(n, G), CC.min_sep_of(G)))
    n, G = 600, 60
    coords = CC.chain(n, cell[0], 2, seed=33).copy()
    coords[:, :, 410] = coords[:, :, 17]
    cases_.append(("shuffled entries, two of them on one point", coords, CC.sites(n, G, seed=2, shuffle=True), 3))
    rng = np.random.default_rng(6)
    big = dict(atoms=np.arange(n, dtype=np.int32), groups=rng.integers(0, 2048, n).astype(np.int32), ngroups=2048)
    cases_.append(("2048 scattered groups", coords, big, 3))
    cases_.append(("2048 groups in list order", coords, dict(big, groups=np.sort(big["groups"])), 3))
    for what, xyz, sites, ms in cases_:
        want = restate(xyz, cell, sites, min_sep=ms)
        assert want["record"][:-1].any(), what
        got = []
        for on in (0, 1):
            with Options(lib, contact_lds_rows=on, **WALK):
                got.append(check(run(lib, sites, xyz, cell, device, min_sep=ms), want, sites, f"{what}, lds rows {on}", list_frames=[]))
        same(got[0], got[1], what)


def test_lds_rows_on_the_emulator(emu_lib):
    lds_rows(emu_lib)


# ---- 3. thresholds and small boxes ------------------------------------------------------------------------------------------------------------

def thresholds(lib, device=False):
    """Two one-atom groups per FRAME on the x axis at r_cut moved by -4 .. 4 ulp, from two positions of the first (coordinates of a few
    Angstrom, so that one ulp is a fine step), under both spec_within_closed settings"""
    frames = []
    for dx in steps(np.float32(CC.R_CUT), -4, 4):
        for base in (5.0, 4.0 + 1.0 / 3.0):
            frames.append([(base, 2.0, 5.0), (float(np.float32(base) + dx), 2.0, 5.0)])
    coords = np.asarray(frames, np.float64).transpose(0, 2, 1).astype(np.float32)
    sites = one_per_group(2)
    cell = ((40.0, 40.0, 40.0), (0.0, 0.0, 0.0), 7)
    got = {}
    for closed in (0, 1):
        want = restate(coords, cell, sites, min_sep=1, closed=bool(closed))
        assert want["near"] >= 8 and 0 < want["record"][0] < len(frames), want["near"]
        got[closed] = all_routes(lib, sites, coords, cell, want, f"thresholds, closed {closed}", device, min_sep=1, spec_within_closed=closed)
    assert got[1][1][0] > got[0][1][0]              # some frame stands at r_cut exactly: the closed test takes it, the open one does not


def test_thresholds_on_the_emulator(emu_lib):
    thresholds(emu_lib)


def tight_boxes(lib, device=False):
    """A cell just large enough for a grid at r_cut (two pencils per axis: every neighbour pencil is met under two images) and one too
    small, where the walk cannot be had and all pairs answer whatever is asked"""
    for edge, grid in ((CC.TIGHT, True), (CC.TOO_SMALL, False)):
        cell = ((edge, edge, edge), (0.0, 0.0, 0.0), 7)
        n, G = 120, 40
        coords = CC.chain(n, cell[0], 2, seed=11)
        sites = CC.sites(n, G)
        want = restate(coords, cell, sites, r=CC.TIGHT_R)
        one = None
        for route in ROUTES:
            lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
            try:
                with Options(lib, **route):
                    got = check(run(lib, sites, coords, cell, device, r=CC.TIGHT_R), want, sites, f"edge {edge}, {route}", list_frames=[0])
            finally:
                lib.vmd_profile_enable(False)
            nw = C.c_uint64(0)
            lib.vmd_profile_ms(b"contact_atoms", C.byref(nw))
            assert (nw.value > 0) == (grid and route is WALK), (edge, route, nw.value)
            one = one or got
            same(got, one, (edge, route))


def test_tight_boxes_on_the_emulator(emu_lib):
    tight_boxes(emu_lib)


# ---- 4. identity ------------------------------------------------------------------------------------------------------------------------------

def identity(lib, device=False):
    cell = CC.CELLS[0]
    n, G = 300, 30
    coords = CC.chain(n, cell[0], 2, seed=5).copy()
    base = CC.sites(n, G)
    want = restate(coords, cell, base)
    one = all_routes(lib, base, coords, cell, want, "contiguous groups", device, list_frames=[1])
    # the bits do not depend on list order: the same entries shuffled give the same record
    shuf = CC.sites(n, G, seed=9, shuffle=True)
    got = all_routes(lib, shuf, coords, cell, restate(coords, cell, shuf), "shuffled entry order", device, list_frames=[1])
    same(got, one, "shuffled against contiguous")
    # groups given in non-contiguous order (the group of an entry has nothing to do with its neighbours in the list), and groups 7 and 29
    # without entries
    rng = np.random.default_rng(3)
    scattered = dict(atoms=base["atoms"], groups=rng.permutation(G)[base["groups"]].astype(np.int32), ngroups=G)
    scattered["groups"][np.isin(scattered["groups"], (7, 29))] = 8
    want = restate(coords, cell, scattered)
    got = all_routes(lib, scattered, coords, cell, want, "scattered groups, two of them empty", device, list_frames=[0])
    P7 = [int(R.pair_index(G, min(7, h), max(7, h))) for h in range(G) if h != 7]
    assert not got[1][P7].any()
    # an atom listed twice in two groups, and two atoms of different groups on one point, bit for bit: D-CT-COINCIDENT, the lowest entry's
    # group acts for both - on either side of a pair
    twice = dict(atoms=np.concatenate([[40], base["atoms"]]).astype(np.int32), groups=np.concatenate([[25], base["groups"]]).astype(np.int32),
                 ngroups=G)
    want = restate(coords, cell, twice)
    all_routes(lib, twice, coords, cell, want, "an atom listed twice in two groups", device, list_frames=[0, 1])
    c2 = coords.copy()
    c2[:, :, 222] = c2[:, :, 17]
    for sites in (base, shuf):
        want = restate(c2, cell, sites)
        all_routes(lib, sites, c2, cell, want, "two entries of different groups on one point", device, list_frames=[0, 1])
    # entries far outside the cell: whole cells (a million of them) move nothing
    far = coords.copy()
    far[:, 0, 0:90] += np.float32(cell[0][0]) * np.float32(1.0e6)
    all_routes(lib, base, far, cell, restate(far, cell, base), "a million cells away", device, list_frames=[0])


def test_identity_on_the_emulator(emu_lib):
    identity(emu_lib)


# ---- 5. the native fraction -------------------------------------------------------------------------------------------------------------------

def sheet_system(F=8):
    """ss_cases.sheet (two antiparallel strands of eight residues, N CA C O each) pulled apart along the direction between the strands'
    centres frame by frame: 0, 0.8, 1.6 ... A"""
    xyz = SS.sheet(False)
    n = xyz.shape[0] // 2
    d = xyz[n:].mean(axis=0) - xyz[:n].mean(axis=0)
    d /= np.linalg.norm(d)
    frames = []
    for f in range(F):
        m = xyz.copy()
        m[n:] += d * (0.8 * f if f < F - 1 else 30.0)
        frames.append(m)
    cell = ((60.0, 60.0, 60.0), (0.0, 0.0, 0.0), 7)
    coords = SS.frames_of(np.stack(frames), cell[0])
    sites = dict(atoms=np.arange(2 * n, dtype=np.int32), groups=(np.arange(2 * n) // 4).astype(np.int32), ngroups=2 * n // 4)
    return coords, cell, sites


def native_q(lib, device=False):
    coords, cell, sites = sheet_system()
    first = run(lib, sites, coords, cell, device, min_sep=1)                     # (min_sep 1: a strand's neighbours count as well)
    native = first.pairs(0)
    G = sites["ngroups"]
    cross = native[(native[:, 0] < G // 2) & (native[:, 1] >= G // 2)]           # the contacts between the strands
    assert len(native) > len(cross) >= 8
    for nat, what in ((native, "all of frame 0"), (cross, "between the strands")):
        want = restate(coords, cell, sites, min_sep=1, native=nat)
        got = all_routes(lib, sites, coords, cell, want, f"sheet pulled apart, natives {what}", device, min_sep=1, native=nat,
                         list_frames=[0, 3])
        q = got[2]
        print(f"Q(t), natives {what}: {q}")
        assert q[0] == np.float32(1.0) and (np.diff(q) <= 0).all() and q[-1] < q[0], q
        # the strands' own contacts stay (the strands move rigidly); those between them all go
        assert q[-1] == (np.float32(len(native) - len(cross)) / np.float32(len(native)) if nat is native else 0.0), q
    # the native list's size edges: the reduction over a wave and a block of native lanes; a pair given as (h, g) is the pair (g, h)
    n, Gc = 257, 64
    ch = CC.chain(n, CC.CELLS[0][0], 3, seed=21)
    st = CC.sites(n, Gc)
    every = run(lib, st, ch, CC.CELLS[0], device)
    seen = np.concatenate([every.pairs(f) for f in range(3)])
    seen = np.unique(seen, axis=0)
    rng = np.random.default_rng(8)
    for nn in CC.NNATIVE:
        nat = seen[rng.permutation(len(seen))[:nn]].copy()
        nat[::2] = nat[::2, ::-1]
        want = restate(ch, CC.CELLS[0], st, native=nat)
        assert 0 < want["q"].sum() and len(nat) == nn
        all_routes(lib, st, ch, CC.CELLS[0], want, f"{nn} native pairs", device, native=nat, list_frames=[])


def test_native_fraction_on_the_emulator(emu_lib):
    native_q(emu_lib)


# ---- 6. call patterns -------------------------------------------------------------------------------------------------------------------------

def call_patterns(lib, device=False):
    """one call; many small ranges in shuffled order; pool threads; clear_data then again; a frame evaluated twice counts twice; a partial
    range (frames never evaluated read +0 and are not counted); a source's frame blocks; the one-frame query touching nothing"""
    cell = CC.CELLS[0]
    n, G, F = 500, 50, 8
    coords = CC.chain(n, cell[0], F, seed=9)
    sites = CC.sites(n, G)
    nat = restate(coords, cell, sites, frames=[0])["pairs"][0][::3]
    want = restate(coords, cell, sites, native=nat)
    kw0 = dict(native=nat)
    with Options(lib, **WALK):
        first = run(lib, sites, coords, cell, device, **kw0)
        one = check(first, want, sites, "one call", list_frames=[0, F - 1])
        order = [(f, f + 1) for f in np.random.default_rng(4).permutation(F)]
        for kw in (dict(ranges=[(5, 8), (0, 2), (2, 5)]), dict(ranges=order), dict(pooled=(16, 1)), dict(pooled=(4, 2))):
            same(run(lib, sites, coords, cell, device, **kw0, **kw).out(), one, kw)
        with Options(lib, batch_frames=3):
            same(run(lib, sites, coords, cell, device, **kw0).out(), one, "batch_frames 3")
        before = first.record()
        first.pairs(3)
        same(first.out(), one, "after the one-frame query")
        assert np.array_equal(first.record(), before)
        first.ev.clear_data()
        assert not first.record().any() and first.ev.contacts(NAMES[1])[1] == 0 and not first.ev.contacts(NAMES[1])[0].any()
        assert first.ev.frame_range(first.sysm, first.traj, 0, F)
        same(first.out(), one, "clear_data, then again")
        part = run(lib, sites, coords, cell, device, ranges=[(2, 5)], **kw0)
        got = check(part, restate(coords, cell, sites, native=nat, frames=[2, 3, 4]), sites, "frames 2 .. 4", list_frames=[2])
        assert not got[0][:2].any() and not got[0][5:].any() and got[1][-1] == 3 and not got[2][:2].any()
        assert part.ev.frame_range(part.sysm, part.traj, 2, 5)
        check(part, restate(coords, cell, sites, native=nat, frames=[2, 3, 4, 2, 3, 4]), sites, "frames 2 .. 4 twice", list_frames=[])
        assert np.array_equal(part.record(), 2 * got[1])
        # a source evaluated in blocks of two frames lends frames 2 .. 3
        ir = ct_ir(lib, sites, native=nat)
        src = V.ScriptEval(F, ir)
        src.set_block_frames(2)
        assert src.frame_range(first.sysm, first.traj, 0, F)
        assert np.array_equal(src.property_data(NAMES[1]).contact_accumulators, one[1])
        flt = V.ScriptEval(F, ir)
        flt.set_block_frames(2)
        flt.set_source(src)
        assert flt.frame_range(first.sysm, first.traj, 2, 4) and flt.frame_stats()[1] > 0
        assert np.array_equal(flt.property_data(NAMES[1]).contact_accumulators,
                              restate(coords, cell, sites, native=nat, frames=[2, 3])["record"])


def test_call_patterns_on_the_emulator(emu_lib):
    call_patterns(emu_lib)


def reader_names(lib, device=False):
    """ScriptEval.contacts under every name of the statement, condensed and square, whatever stands next to the statement in the IR: an
    rmsf record (a MAP) directly behind the native fraction - of 3 atoms, whose 4 rows are 1 + a triangular number, and of 4 - and an
    hbonds occupancy (a MAP) directly in front of the count"""
    cell = CC.CELLS[0]
    n, G = 120, 5
    coords = CC.chain(n, cell[0], 3, seed=19)
    sites = CC.sites(n, G)
    nat = np.array([[0, 2], [4, 1]], np.int32)
    want = restate(coords, cell, sites, min_sep=1, native=nat)
    assert want["record"][:-1].any()
    for nfl in (3, 4):
        ir = V.ScriptIR(lib)
        ir.add_hbonds(("nhb", "occ"), [0, 3], [1, 4], [0, 3, 6], 3.5, 150.0)
        ir.add_contacts(NAMES + (QNAME,), sites["atoms"], sites["groups"], CC.R_CUT, 1, native=nat, ngroups=G)
        ir.add_rmsf("fl", np.arange(nfl, dtype=np.int32))
        assert ir.property_names() == ["nhb", "occ", "nc", "cmap", "q", "fl"]
        rn = Run(lib, ir, coords, cell, device)
        assert np.array_equal(rn.record(), want["record"])
        F = int(want["record"][-1])
        occ = want["record"][:-1] / F
        for nm in NAMES + (QNAME,):
            got, frames = rn.ev.contacts(nm)
            assert frames == F and got.shape == (G * (G - 1) // 2,) and np.array_equal(got, occ), (nfl, nm)
            sq, frames = rn.ev.contacts(nm, square=True)
            assert frames == F and sq.shape == (G, G) and np.array_equal(sq, sq.T) and not np.diag(sq).any(), (nfl, nm)
            assert np.array_equal(sq[np.triu_indices(G, 1)], occ), (nfl, nm)
        for nm in ("fl", "occ", "nhb"):
            with pytest.raises(V.VmdError, match="not a contacts property"):
                rn.ev.contacts(nm)


def test_reader_under_every_name_on_the_emulator(emu_lib):
    reader_names(emu_lib)


def overflow_case(lib, O, device=False):
    """test_hbond.overflow_case's construction: the middle frames pile every oxygen into one pencil, a bucket sized from the batch's ends
    overflows and the batch is repeated.  The record is added to behind the overflow flag: it must not count that batch twice - the record
    is that of an IR without the rdf, which no overflow ever touches (all pairs)."""
    n, box, F = 3000, 60.0, 12
    coords = cases.water_box(O, 5, n, box, F)
    o = cases.oxygen(n)
    rng = np.random.default_rng(3)
    for f in (5, 6, 7):
        coords[f][:, o] = rng.uniform(1.0, 11.0, (3, o.size)).astype(np.float32)
    ent = o[:600]
    sites = dict(atoms=ent.astype(np.int32), groups=(np.arange(ent.size) // 3).astype(np.int32), ngroups=200)
    cell = ((box, box, box), (0.0, 0.0, 0.0), 7)
    with Options(lib, **BRUTE):
        alone = run(lib, sites, coords, cell, device)
    one = alone.out()
    assert one[1][-1] == F and one[1][:-1].any()
    with Options(lib, cells_small=0, cells_cap_sample=2, **WALK):
        for bf in (0, 4):
            with Options(lib, batch_frames=bf):
                ir = ct_ir(lib, sites)
                ir.add_rdf("goo", o, o, (0.0, 12.0))
                lib.vmd_profile_reset(); lib.vmd_profile_enable(True)
                try:
                    rn = Run(lib, ir, coords, cell, device)
                finally:
                    lib.vmd_profile_enable(False)
                nb = C.c_uint64(0)
                lib.vmd_profile_ms(b"cells_build", C.byref(nb))
                assert nb.value > 2 * ((F + bf - 1) // bf if bf else 1), "no batch was rebuilt"
                lib.vmd_profile_ms(b"contact_atoms", C.byref(nb))
                assert nb.value > ((F + bf - 1) // bf if bf else 1), "the walk of the repeated batch did not run again"
                same(rn.out(), one, bf)
    check(alone, restate(coords, cell, sites), sites, "next to an rdf that repeats its batch", list_frames=[6])


def test_next_to_an_rdf_that_repeats_its_batch(emu_lib, oracle):
    overflow_case(emu_lib, oracle)


# ---- 7. the two-rank merge ------------------------------------------------------------------------------------------------------------------

def _merge_case():
    coords = CC.chain(300, CC.CELLS[0][0], 6, seed=13)
    sites = CC.sites(300, 40)
    return coords, sites, np.array([[0, 3], [5, 9], [2, 30], [10, 14]], np.int32)


def _merge_worker(rank, world, port, tmpdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import conftest
    from viamd_amd.dist import reduce_eval, shard_frames
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lib = V.VmdLib(conftest.EMU_LIB)
    coords, sites, nat = _merge_case()
    F = coords.shape[0]
    ev = V.ScriptEval(F, ct_ir(lib, sites, native=nat))
    beg, end = shard_frames(F, rank, world)
    cell = V.make_unitcell(CC.CELLS[0][0])
    assert ev.frame_range(V.MolSystem(coords.shape[2], unitcell=cell), V.HostTrajectory(coords, cell), beg, end)
    own = ev.property_data(NAMES[1]).contact_accumulators.copy()
    reduce_eval(ev)
    occ, frames = ev.contacts(NAMES[1])
    np.savez(os.path.join(tmpdir, f"rank{rank}.npz"), own=own, merged=ev.property_data(NAMES[1]).contact_accumulators.copy(),
             counts=TG.rows(ev, NAMES[0])[:, 0], q=TG.rows(ev, QNAME)[:, 0], occ=occ, frames=frames)
    dist.destroy_process_group()


def test_two_rank_merge(emu_lib, tmp_path):
    """two evals over the halves of the frames, merged through the host collective: every rank's merged record, counts and Q are the
    one-rank ones bit for bit"""
    import torch.multiprocessing as mp
    port = 53700 + (os.getpid() % 2000)
    mp.spawn(_merge_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    coords, sites, nat = _merge_case()
    rn = run(emu_lib, sites, coords, CC.CELLS[0], native=nat)
    check(rn, restate(coords, CC.CELLS[0], sites, native=nat), sites, "one rank", list_frames=[0])
    total = np.zeros_like(rn.record())
    for r in range(2):
        z = np.load(tmp_path / f"rank{r}.npz")
        total = total + z["own"]
        assert np.array_equal(z["merged"], rn.record()) and int(z["frames"]) == coords.shape[0]
        assert np.array_equal(z["counts"].view(np.int32), rn.counts().view(np.int32))
        assert np.array_equal(z["q"].view(np.int32), rn.q().view(np.int32))
        assert np.array_equal(z["occ"], rn.ev.contacts(NAMES[1])[0])
    assert np.array_equal(total, rn.record())


# ---- 8. the topology helper -------------------------------------------------------------------------------------------------------------------

class _Topo:
    def __init__(self, elements, residue_index=None):
        self.elements = np.array(elements)
        self.num_atoms = len(elements)
        self.residue_index = None if residue_index is None else np.asarray(residue_index, np.int64)


def test_contact_sites_from_topology(host_lib):
    water = _Topo(["O", "H", "H"] * 3, np.repeat([0, 1, 2], 3))
    for got in (script.contact_sites_from_topology(water), script.contact_sites_from_topology_native(water, lib=host_lib)):
        assert list(got["atoms"]) == [0, 3, 6] and list(got["groups"]) == [0, 1, 2] and got["ngroups"] == 3
        assert got["atoms"].dtype == np.int32 and got["groups"].dtype == np.int32
    for got in (script.contact_sites_from_topology(water, False), script.contact_sites_from_topology_native(water, False, lib=host_lib)):
        assert list(got["atoms"]) == list(range(9)) and list(got["groups"]) == [0, 0, 0, 1, 1, 1, 2, 2, 2] and got["ngroups"] == 3
    # a hand-written peptide: residue numbers that start at 7, skip and come back; a lower-case hydrogen; a residue of hydrogens only
    pep = _Topo(["N", "h", "C", "C", "O", "N", "H", "C", "H", "H", "S", "C"], [7, 7, 7, 7, 7, 9, 9, 9, 4, 4, 12, 7])
    for got in (script.contact_sites_from_topology(pep), script.contact_sites_from_topology_native(pep, lib=host_lib)):
        assert list(got["atoms"]) == [0, 2, 3, 4, 5, 7, 10, 11] and list(got["groups"]) == [0, 0, 0, 0, 1, 1, 2, 0] and got["ngroups"] == 3
    for got in (script.contact_sites_from_topology(pep, False), script.contact_sites_from_topology_native(pep, False, lib=host_lib)):
        assert list(got["groups"]) == [0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 0] and got["ngroups"] == 4
    # no residue_index: one group - which the entry point refuses, not the helper
    bare = _Topo(["C", "H", "O"])
    for got in (script.contact_sites_from_topology(bare), script.contact_sites_from_topology_native(bare, lib=host_lib)):
        assert list(got["atoms"]) == [0, 2] and list(got["groups"]) == [0, 0] and got["ngroups"] == 1
        with pytest.raises(V.VmdError, match=r"\[2, 2048\]"):
            V.ScriptIR(host_lib).add_contacts(NAMES, got["atoms"], got["groups"], ngroups=got["ngroups"], min_sep=1)
    assert not host_lib.vmd_topology_contact_sites(None, True) and "NULL" in host_lib.last_error()


# ---- 9. the IR: every refusal, the fingerprint field by field, the statement next to the others ---------------------------------------------

def test_ir_validation_errors(host_lib):
    lib = host_lib
    for sym in ("vmd_ir_add_contacts", "vmd_eval_contacts", "vmd_eval_contact_pairs", "vmd_topology_contact_sites", "vmd_contact_sites_view",
                "vmd_contact_sites_free", "vmd_hip_contact_atoms", "vmd_hip_contact_brute", "vmd_hip_contact_finish"):
        assert hasattr(lib, sym), sym
    ir = V.ScriptIR(lib)
    ok = dict(atoms=[0, 1, 2, 3, 4, 5], groups=[0, 0, 1, 2, 3, 4], r_cut=4.5, min_sep=2, ngroups=5)

    def bad(match, names=NAMES, **kw):
        a = dict(ok, **kw)
        nm = tuple(names) + ((QNAME,) if a.get("native") is not None and len(a["native"]) and len(names) == 2 else ())
        with pytest.raises(V.VmdError, match=match):
            ir.add_contacts(nm, **a)
    bad("entry list is empty", atoms=[], groups=[])
    bad("negative", atoms=[0, 1, 2, 3, 4, -5])
    bad("names group -1", groups=[0, 0, 1, 2, 3, -1])
    bad("names group 5", groups=[0, 0, 1, 2, 3, 5])
    for G in (0, 1, 2049, 1 << 20):
        bad(r"\[2, 2048\]", ngroups=G, groups=[0] * 6, min_sep=1)
    for r in (0.0, -1.0, float("inf"), float("nan")):
        bad("cutoff must be finite and positive", r_cut=r)
    for ms in (0, 5, 1000):
        bad(r"minimum separation must lie in \[1, 4\]", min_sep=ms)
    bad("names group 2 twice", native=[[0, 3], [2, 2]])
    bad("outside", native=[[0, 5]])
    bad("outside", native=[[-1, 3]])
    bad("closer than the minimum separation", native=[[0, 2], [3, 4]])
    bad("listed twice", native=[[0, 2], [1, 4], [0, 2]])
    bad("listed twice", native=[[0, 2], [2, 0]])
    bad("name is empty", names=("", "cmap"))
    bad("already defined", names=("x", "x"))
    bad("already defined", names=("nc", "cmap", "nc"), native=[[0, 2]])
    names3 = (C.c_char_p * 3)(b"a", b"b", b"c")
    names2 = (C.c_char_p * 3)(b"a", b"b", None)
    at, gr = (np.array(v, np.int32) for v in ([0, 1], [0, 1]))
    nat = np.array([[0, 1]], np.int32)
    ip = lambda x: x.ctypes.data_as(L.c_int32_p)
    sites = L.ContactSitesC(2, ip(at), ip(gr), 2, 0, None)
    with_nat = L.ContactSitesC(2, ip(at), ip(gr), 2, 1, ip(nat))
    assert not lib.vmd_ir_add_contacts(None, names2, C.byref(sites), 4.5, 1) and "ir is NULL" in lib.last_error()
    assert not lib.vmd_ir_add_contacts(ir.h, None, C.byref(sites), 4.5, 1) and "property names" in lib.last_error()
    assert not lib.vmd_ir_add_contacts(ir.h, names2, None, 4.5, 1) and "the sites" in lib.last_error()
    assert not lib.vmd_ir_add_contacts(ir.h, names3, C.byref(sites), 4.5, 1) and "third must be NULL" in lib.last_error()
    assert not lib.vmd_ir_add_contacts(ir.h, names2, C.byref(with_nat), 4.5, 1) and "third property name" in lib.last_error()
    assert not lib.vmd_ir_add_contacts(ir.h, names3, C.byref(L.ContactSitesC(2, ip(at), ip(gr), 2, 1, None)), 4.5, 1) and "NULL" in lib.last_error()
    for s in (L.ContactSitesC(2, None, ip(gr), 2, 0, None), L.ContactSitesC(2, ip(at), None, 2, 0, None)):
        assert not lib.vmd_ir_add_contacts(ir.h, names2, C.byref(s), 4.5, 1) and "empty" in lib.last_error()
    assert ir.property_count() == 0                                                # a refused statement leaves nothing behind
    ir.add_rmsd("g", [0, 1])
    bad("already defined", names=("g", "cmap"))
    bad("already defined", names=("nc", "g"))
    bad("already defined", names=("nc", "cmap", "g"), native=[[0, 2]])
    ir.add_contacts(NAMES + (QNAME,), **dict(ok, native=[[4, 0], [1, 3]]))
    ir.add_contacts(("n1", "m1"), **dict(ok, min_sep=1))                           # the ends of the range
    ir.add_contacts(("n4", "m4"), **dict(ok, min_sep=4))
    with pytest.raises(V.VmdError, match="already defined"):
        ir.add_rmsd("cmap", [0, 1])
    assert ir.property_names()[:4] == ["g", "nc", "cmap", "q"]
    assert ir.property_flags("nc") == L.FLAG_TEMPORAL and ir.property_flags("cmap") == L.FLAG_MAP and ir.property_flags("q") == L.FLAG_TEMPORAL
    with pytest.raises(ValueError):
        V.ScriptIR(lib).add_contacts(NAMES, [0, 1], [0])
    ir2 = V.ScriptIR(lib)
    ir2.add_contacts(NAMES, [0, 99], [0, 1], min_sep=1)
    # (what follows evaluates: the emulator build always gets here, the product library only where there is a device)
    if lib.vmd_device_count() > 0:
        cell = ((10.0, 10.0, 10.0), (0.0, 0.0, 0.0), 7)
        with pytest.raises(V.VmdError, match="references atom 99"):
            Run(lib, ir2, np.zeros((1, 3, 10), np.float32), cell)
        rn = Run(lib, ir, np.zeros((2, 3, 10), np.float32), cell)
        ev = rn.ev
        with pytest.raises(V.VmdError, match="not a contacts property"):
            ev.contacts("g")
        with pytest.raises(V.VmdError, match="not a contacts property"):
            ev.contact_pairs("g", rn.sysm, rn.traj, 0)
        with pytest.raises(V.VmdError, match="outside the trajectory"):
            ev.contact_pairs("nc", rn.sysm, rn.traj, 2)
        assert not lib.vmd_eval_contacts(ev.h, b"nope", None, None) and "unknown property" in lib.last_error()
        assert not lib.vmd_eval_contacts(None, b"cmap", None, None) and "NULL" in lib.last_error()
        failed = C.c_size_t(-1).value
        assert lib.vmd_eval_contact_pairs(ev.h, b"nope", None, rn.traj.interface(), 0, None, 0) == failed
        assert lib.vmd_eval_contact_pairs(None, b"cmap", None, rn.traj.interface(), 0, None, 0) == failed
        # all atoms at the origin: every entry coincides with entry 0 and acts for group 0 - no two groups, no pair, under every name
        for nm in (b"nc", b"cmap", b"q"):
            assert lib.vmd_eval_contact_pairs(ev.h, nm, None, rn.traj.interface(), 0, None, 0) == 0
            assert lib.vmd_eval_contacts(ev.h, nm, None, None)
        pd = ev.property_data("cmap")
        assert pd.dim == (11, 1, 0, 0) and pd.unit_str == ("", "") and list(pd.contact_accumulators) == [0] * 10 + [2]
        assert ev.property_data("nc").dim == (2, 1, 0, 0) and ev.property_data("q").dim == (2, 1, 0, 0)
        with pytest.raises(V.VmdError, match="record of a contact map"):
            ev.export_table("/dev/null", "cmap", "csv")


def test_fingerprint_work_and_atoms(host_lib):
    assert TR._old_ir(host_lib).fingerprint() == TR.PARENT_FINGERPRINT              # an IR without the forms keeps its fingerprint

    def fp(**kw):
        ir = V.ScriptIR(host_lib)
        a = dict(names=NAMES + (QNAME,), atoms=[0, 1, 2, 3, 4, 5], groups=[0, 0, 1, 2, 3, 4], r_cut=4.5, min_sep=2, ngroups=5,
                 native=[[0, 2], [1, 4]])
        a.update(kw)
        if a["native"] is None:
            a["names"] = a["names"][:2]
        ir.add_contacts(**a)
        return ir.fingerprint(), int(host_lib.vmd_ir_work_per_frame(ir.h))
    f0, w0 = fp()
    variants = dict(name0=fp(names=("x", "cmap", "q")), name1=fp(names=("nc", "x", "q")), name2=fp(names=("nc", "cmap", "x")),
                    atoms=fp(atoms=[0, 1, 2, 3, 4, 6]), order=fp(atoms=[1, 0, 2, 3, 4, 5]), groups=fp(groups=[0, 1, 1, 2, 3, 4]),
                    fewer=fp(atoms=[0, 1, 2, 3, 4], groups=[0, 1, 2, 3, 4]), ngroups=fp(ngroups=6), r_cut=fp(r_cut=4.6), min_sep=fp(min_sep=1),
                    moved=fp(native=[[0, 2], [1, 3]]), swapped=fp(native=[[1, 4], [0, 2]]), fewer_native=fp(native=[[0, 2]]),
                    no_native=fp(native=None))
    assert len({f0} | {v[0] for v in variants.values()}) == 1 + len(variants), variants
    assert fp(native=[[2, 0], [4, 1]])[0] == f0                                     # a pair is a pair in either order
    assert w0 == 4 * 6 and variants["fewer"][1] == 4 * 5
    # hbonds over the same atoms is another statement
    ir = V.ScriptIR(host_lib)
    ir.add_hbonds(NAMES, [0, 3], [1, 4], [0, 1, 3], 3.5, 150.0)
    assert ir.fingerprint() != f0
    ir = TR._old_ir(host_lib)
    w_old = int(host_lib.vmd_ir_work_per_frame(ir.h))
    ir.add_contacts(NAMES, [0, 3, 5], [0, 1, 2], min_sep=1)
    assert ir.fingerprint() != TR.PARENT_FINGERPRINT and int(host_lib.vmd_ir_work_per_frame(ir.h)) == w_old + 12
    assert list(ir.geometry_atoms("nc")) == [0, 3, 5] and list(ir.geometry_atoms("nc", 0)) == [0, 3, 5]
    assert ir.geometry_atoms("nc", 1).size == 0 and ir.geometry_atoms("cmap").size == 0


def next_to_the_other_forms(lib, oracle, device=False):
    """VIAMD's default script plus rmsd, ramachandran, secondary_structure, rmsf, hbonds and sasa statements, with and without a contacts
    statement in the same IR: every other property is bit-identical, the new ones equal the restatement and an IR of their own"""
    atoms, blob, box, F = 6001, 200, 30.0, 4
    coords, topo = TG.blob_system(oracle, n_atoms=atoms, n_blob=blob, box=box, F=F, seed=5)
    names = np.array(["N", "CA", "C", "O", "CB", "H", "HA", "HB1", "CG", "HG"])
    topo.names = np.where(np.arange(atoms) < blob, names[np.arange(atoms) % 10], topo.elements)
    bb = script.backbone_from_topology(topo)
    o = script.backbone_oxygens_from_topology(topo, bb)
    el = np.array([str(e).upper() for e in topo.elements])
    wo = np.nonzero((el == "O") & (np.arange(atoms) >= blob))[0]
    bonds = [(int(i), int(i) + k) for i in wo for k in (1, 2) if i + k < atoms and el[i + k] == "H"]
    hb = script.hbond_sites_from_topology(topo, bonds)
    rad = script.vdw_radii_from_topology(topo)
    all_sites = script.contact_sites_from_topology(topo, heavy_only=True)
    keep = all_sites["atoms"] < blob                                                # the blob's residues, heavy atoms
    sites = dict(atoms=all_sites["atoms"][keep], groups=all_sites["groups"][keep], ngroups=int(all_sites["groups"][keep].max()) + 1)
    assert sites["ngroups"] >= 10
    cell = ((box, box, box), (0.0, 0.0, 0.0), 7)
    native = restate(coords, cell, sites, frames=[0])["pairs"][0]
    assert len(native) > 0
    evs = []
    for with_contacts in (False, True):
        ir = script.compile_script_native(TG.VIAMD_DEFAULT_SCRIPT + TR.RM_LINE, topo, lib=lib, **OPT_INS)
        ir.add_ramachandran(("bb", "rama"), **bb)
        ir.add_secondary_structure(("ss", "sspop"), bb["n"], bb["ca"], bb["c"], o, bb["range_offsets"], bb["rama_class"])
        ir.add_rmsf("fl", np.arange(blob, dtype=np.int32))
        ir.add_hbonds(("nhb", "occ"), hb["donor"], hb["hydrogen"], hb["acceptor"], HC.R_DA, HC.ANGLE)
        ir.add_sasa(("area", "pts"), np.arange(atoms, dtype=np.int32), rad, measured=np.arange(blob))
        if with_contacts:
            ir.add_contacts(NAMES + (QNAME,), sites["atoms"], sites["groups"], CC.R_CUT, CC.MIN_SEP, native=native, ngroups=sites["ngroups"])
        evs.append(TG.evaluate(lib, ir, coords, box, topo.mass, device=device))
    plain, both = evs
    props = plain.ir.property_names()
    assert props == ["d1", "a1", "r", "v", "lin", "plan", "iso", "rm", "bb", "rama", "ss", "sspop", "fl", "nhb", "occ", "area", "pts"]
    assert both.ir.property_names() == props + list(NAMES) + [QNAME]
    for name in props:
        a, b = plain.property_data(name), both.property_data(name)
        assert a.dim == b.dim and a.fingerprint == b.fingerprint, name
        assert np.array_equal(a.values.view(np.int32), b.values.view(np.int32)), name
        if a.c.counts:
            assert np.array_equal(a.counts, b.counts), name
    want = restate(coords, cell, sites, native=native)
    print(f"blob system: {int(want['record'][:-1].sum())} contacts, {want['near']} candidate entry pairs within 4 ulp of r_cut, Q {want['q']}")
    assert want["q"][0] == 1.0
    got = (TG.rows(both, NAMES[0])[:, 0], both.property_data(NAMES[1]).contact_accumulators, TG.rows(both, QNAME)[:, 0])
    assert np.array_equal(got[0].view(np.int32), want["counts"].view(np.int32)) and np.array_equal(got[1], want["record"])
    assert np.array_equal(got[2].view(np.int32), want["q"].view(np.int32))
    alone = run(lib, sites, coords, cell, device, native=native)
    same(alone.out(), got, "an IR of its own")


def test_next_to_the_other_forms_on_the_emulator(emu_lib, oracle):
    next_to_the_other_forms(emu_lib, oracle)


# ---- 10. the equality was exercised -----------------------------------------------------------------------------------------------------------

def test_zz_thresholds_were_met(emu_lib):
    """the threshold scenarios did produce candidate pairs within 4 ulp of r_cut (run on their own when this test is selected alone)"""
    if not any(k.startswith("thresholds") for k in NEAR):
        thresholds(emu_lib)
    met = {k: v for k, v in NEAR.items() if k.startswith("thresholds")}
    print(met)
    assert met and all(v >= 8 for v in met.values())
