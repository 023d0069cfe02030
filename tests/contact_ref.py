"""Independent restatement of DESIGN 1.16 - residue contact maps and the native-contact fraction - in numpy.

It imports neither the package nor the oracle.  All pairs, no cells, fp32 operation by operation: the wrap of tests/within_ref.py, the delta
and the coincidence rule of tests/hbond_ref.py (D-HB-DISTANCE, D-HB-COINCIDENT, word for word).  One list of entries (atom, group):
  1. every entry is wrapped (SPEC S2 / S3t); an entry ACTS for the group of the lowest list entry whose wrapped coordinates equal its own
     bit for bit (D-CT-COINCIDENT) - on either side of a pair;
  2. entries i, j are in range when e = (i - j) - shift with the SPEC S3 / S3t image, d2 = fmaf(ez, ez, fmaf(ey, ey, ex ex)),
     d = sqrtf(d2), 0 <= d < r_cut (closed: <= r_cut);
  3. groups g < h are in contact in the frame iff h - g >= min_sep and some entry acting for g is in range of some entry acting for h.
Pair (g, h) has the condensed index p = g (2 G - g - 1) / 2 + (h - g - 1) (SciPy's pdist order).  Per frame: the number of pairs in
contact as a float32; Q = float32(n) / float32(nnative), n the native pairs in contact.  The record: u64 [P + 1], row p the evaluated frames
with pair p in contact, the last row the frames.
near: how many candidate entry pairs (i < j, their groups a pair at all) lie within 4 ulp of r_cut."""
import numpy as np

from geometry_ref import Box
from hbond_ref import canonical, delta, ulps_between
from within_ref import fmaf, wrap

f32 = np.float32


def pair_index(G, g, h):
    g, h = np.asarray(g, np.int64), np.asarray(h, np.int64)
    return g * (2 * G - g - 1) // 2 + (h - g - 1)


def frame_map(xyz, box, atoms, groups, G, r_cut, min_sep, closed=False, chunk=256):
    """one frame -> (contact bool [G, G], upper triangle; near)"""
    atoms, groups = np.asarray(atoms, np.int64), np.asarray(groups, np.int64)
    r_cut = f32(r_cut)
    aw = wrap(xyz[:, atoms], box)
    g_eff = groups[canonical(aw)]
    contact = np.zeros((G, G), bool)
    near = 0
    for a in range(0, atoms.size, chunk):
        sl = slice(a, a + chunk)
        e = delta(box, aw[:, sl, None], aw[:, None, :])
        d2 = fmaf(e[2], e[2], fmaf(e[1], e[1], e[0] * e[0]))
        d = np.sqrt(d2.astype(np.float32))
        hit = (d <= r_cut) if closed else (d < r_cut)
        gi, gj = g_eff[sl, None], g_eff[None, :]
        pair = np.abs(gi - gj) >= min_sep
        upper = np.arange(a, min(a + chunk, atoms.size))[:, None] < np.arange(atoms.size)[None, :]
        near += int((pair & upper & (ulps_between(d, r_cut) <= 4)).sum())
        ii, jj = np.nonzero(hit & pair)
        lo, hi = np.minimum(g_eff[a + ii], g_eff[jj]), np.maximum(g_eff[a + ii], g_eff[jj])
        contact[lo, hi] = True
    return contact, near


def evaluate(coords, box, atoms, groups, G, r_cut, min_sep, native=None, closed=False, flags=7, frames=None):
    """coords float32 [F, 3, N]; frames: the evaluated frames in order, a frame named twice counts twice.
    -> dict(counts float32 [F] (0 where not evaluated), q float32 [F] (None without natives), record uint64 [P + 1],
            pairs {frame: int32 [n, 2] group pairs in ascending condensed index}, near)"""
    F = coords.shape[0]
    frames = list(range(F)) if frames is None else list(frames)
    P = G * (G - 1) // 2
    rec = np.zeros(P + 1, np.uint64)
    counts = np.zeros(F, np.float32)
    nat = None if native is None or len(native) == 0 else np.sort(np.asarray(native, np.int64).reshape(-1, 2), axis=1)
    q = None if nat is None else np.zeros(F, np.float32)
    pairs = {}
    near = 0
    for f in frames:
        bx = Box(box[f] if isinstance(box, list) else box, flags)
        contact, nd = frame_map(coords[f], bx, atoms, groups, G, r_cut, min_sep, closed)
        near += nd
        g, h = np.nonzero(contact)          # row-major over the upper triangle: ascending condensed index
        assert (g < h).all()
        counts[f] = f32(g.size)
        rec[pair_index(G, g, h)] += np.uint64(1)
        rec[P] += np.uint64(1)
        pairs[f] = np.stack([g, h], axis=1).astype(np.int32)
        if nat is not None:
            q[f] = f32(int(contact[nat[:, 0], nat[:, 1]].sum())) / f32(nat.shape[0])
    return dict(counts=counts, q=q, record=rec, pairs=pairs, near=near)
