"""Restatement of DESIGN 1.12 (per-frame secondary structure) in numpy, written out from the contract text.

Vectors between atoms are fp32 minimum-image differences of raw positions (geometry_ref.Box.mi_f32); everything after that is fp64, one
operation at a time in the written order.  The H-bond matrix is formed for all (acceptor, donor) pairs at once - the same IEEE operations
element by element -; turns, bridges, ladders and the seven assignment passes are taken literally, residue by residue, with no bit
tricks.  It imports neither the package nor the oracle.
"""
import numpy as np

import geometry_ref as G

UNKNOWN, COIL, TURN, BEND, HELIX_310, HELIX_ALPHA, HELIX_PI, BETA_BRIDGE, BETA_SHEET = range(9)
NUM_CODES = 9
LETTERS = "?-TSGHIBE"
COS70 = 0.3420201433256687


def ranges_of(nseg, range_offsets):
    off = np.asarray(range_offsets, np.int64)
    assert off[0] == 0 and off[-1] == nseg and (np.diff(off) > 0).all()
    rng = np.zeros(nseg, np.int64)
    for r in range(off.size - 1):
        rng[off[r]:off[r + 1]] = r
    return rng


def _len(v):
    x, y, z = (np.asarray(k, np.float64) for k in v)
    return np.sqrt((x * x + y * y) + z * z)


def _diff(bx, p, q):
    """mi(p - q), fp32, for position arrays [..., 3] that broadcast"""
    return bx.mi_f32(p[..., 0] - q[..., 0], p[..., 1] - q[..., 1], p[..., 2] - q[..., 2])


def frame_details(xyz, bx, n, ca, c, o, rng, pro):
    """xyz float32 [N, 3] -> dict(hb [a, d], donor, energy [a, d] (nan where not evaluated), gate2 [a, d])"""
    nseg = n.size
    linked = lambda i, j: 0 <= i < nseg and 0 <= j < nseg and rng[i] == rng[j]
    N, CA, C = xyz[n], xyz[ca], xyz[c]
    O = xyz[np.maximum(o, 0)]
    has_o = o >= 0
    # D-SS-H
    donor = np.zeros(nseg, bool)
    u = np.zeros((nseg, 3))
    for d in range(nseg):
        if not (linked(d, d - 1) and not pro[d] and has_o[d - 1]):
            continue
        v = _diff(bx, C[d - 1], O[d - 1])
        l = _len(v)
        if l > 0:
            donor[d] = True
            u[d] = [np.float64(v[0]) / l, np.float64(v[1]) / l, np.float64(v[2]) / l]
    # D-SS-HBOND over all (a, d)
    a_, d_ = np.arange(nseg)[:, None], np.arange(nseg)[None, :]
    same = rng[:, None] == rng[None, :]
    g = _diff(bx, CA[None, :, :], CA[:, None, :])
    gx, gy, gz = (np.asarray(k, np.float64) for k in g)
    gate2 = (gx * gx + gy * gy) + gz * gz
    ev = (a_ != d_) & ~((d_ == a_ + 1) & same) & has_o[:, None] & donor[None, :] & (gate2 < 81.0)
    ON = [np.asarray(k, np.float64) for k in _diff(bx, N[None, :, :], O[:, None, :])]
    CN = [np.asarray(k, np.float64) for k in _diff(bx, N[None, :, :], C[:, None, :])]
    OH = [ON[k] + u[None, :, k] for k in range(3)]
    CH = [CN[k] + u[None, :, k] for k in range(3)]
    rON, rCN, rOH, rCH = _len(ON), _len(CN), _len(OH), _len(CH)
    with np.errstate(divide="ignore", invalid="ignore"):
        energy = 27.888 * (((1.0 / rON + 1.0 / rCH) - 1.0 / rOH) - 1.0 / rCN)
    close = (rON < 0.5) | (rCN < 0.5) | (rOH < 0.5) | (rCH < 0.5)
    hb = ev & (close | (energy < -0.5))
    return dict(hb=hb, donor=donor, energy=np.where(ev, energy, np.nan), gate2=gate2, evaluated=ev, r=(rON, rCH, rOH, rCN))


def frame_classes(xyz, bx, n, ca, c, o, rng, pro, details=None):
    """one frame -> uint8 [nseg]; `details` (a dict) receives hb, par, anti, ladder, turns"""
    nseg = n.size
    det = frame_details(xyz, bx, n, ca, c, o, rng, pro)
    HB = det["hb"]
    inside = lambda i: 0 <= i < nseg
    linked = lambda i, j: inside(i) and inside(j) and rng[i] == rng[j]
    hb = lambda a, d: inside(a) and inside(d) and bool(HB[a, d])
    turn = {k: np.array([linked(i, i + k) and hb(i, i + k) for i in range(nseg)], bool) for k in (3, 4, 5)}
    both = np.array([linked(i, i - 1) and linked(i, i + 1) for i in range(nseg)], bool)
    par, anti = np.zeros((nseg, nseg), bool), np.zeros((nseg, nseg), bool)
    for i in np.flatnonzero(both):
        for j in np.flatnonzero(both):
            if rng[i] == rng[j] and abs(int(i) - int(j)) < 3:
                continue
            par[i, j] = (hb(i - 1, j) and hb(j, i + 1)) or (hb(j - 1, i) and hb(i, j + 1))
            anti[i, j] = (hb(i, j) and hb(j, i)) or (hb(i - 1, j + 1) and hb(j - 1, i + 1))
    P = lambda i, j: inside(i) and inside(j) and bool(par[i, j])
    A = lambda i, j: inside(i) and inside(j) and bool(anti[i, j])
    ladder = np.zeros(nseg, bool)
    for i in range(nseg):
        for j in np.flatnonzero(par[i] | anti[i]):
            if (P(i, j) and (P(i + 1, j + 1) or P(i - 1, j - 1))) or (A(i, j) and (A(i + 1, j - 1) or A(i - 1, j + 1))):
                ladder[i] = True
    # the seven passes; 0 = unassigned
    code = np.zeros(nseg, np.uint8)
    bridge = par.any(axis=1) | anti.any(axis=1)
    code[bridge] = BETA_BRIDGE
    code[bridge & ladder] = BETA_SHEET
    for k, helix, over in ((4, HELIX_ALPHA, True), (3, HELIX_310, False), (5, HELIX_PI, False)):
        before = code.copy()
        for i in range(1, nseg):
            if turn[k][i - 1] and turn[k][i] and (over or not before[i:i + k].any()):
                code[i:i + k] = helix
    before = code.copy()
    for i in range(nseg):
        if before[i]:
            continue
        if any(inside(i - k) and turn[m][i - k] for m in (3, 4, 5) for k in range(1, m)):
            code[i] = TURN
            continue
        code[i] = COIL
        if linked(i, i - 2) and linked(i, i + 2):
            a = [np.float64(v) for v in _diff(bx, xyz[ca[i]], xyz[ca[i - 2]])]
            b = [np.float64(v) for v in _diff(bx, xyz[ca[i + 2]], xyz[ca[i]])]
            aa, bb = G._dot(a, a), G._dot(b, b)
            if aa * bb > 0 and G._dot(a, b) / np.sqrt(aa * bb) < COS70:
                code[i] = BEND
    if details is not None:
        details.update(det, par=par, anti=anti, ladder=ladder, turn=turn)
    return code


def classes(coords, box, n, ca, c, o, range_offsets, rama_class=None, flags=7, details=None):
    """coords float32 [F, 3, N]; box as geometry_ref.Box takes it -> uint8 [F, nseg]; details: a list that receives one dict per frame"""
    n, ca, c, o = (np.asarray(v, np.int64) for v in (n, ca, c, o))
    nseg = n.size
    rng = ranges_of(nseg, range_offsets)
    pro = np.zeros(nseg, bool) if rama_class is None else np.asarray(rama_class) == 2
    bx = G.Box(box, flags)
    out = np.zeros((coords.shape[0], nseg), np.uint8)
    for f in range(coords.shape[0]):
        det = {} if details is not None else None
        out[f] = frame_classes(np.asarray(coords[f], np.float32).T, bx, n, ca, c, o, rng, pro, det)
        if details is not None:
            details.append(det)
    return out


def populations(codes):
    """uint8 [F, nseg] -> float32 [F, 9]"""
    return np.stack([np.bincount(row, minlength=NUM_CODES)[:NUM_CODES] for row in codes]).astype(np.float32)


def letters(row):
    return "".join(LETTERS[int(k)] for k in row)
