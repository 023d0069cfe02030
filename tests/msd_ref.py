"""NumPy restatement of DESIGN 1.18 (mean-squared displacement over lag times): the position table's rows, the time unwrap in integers
(D-MSD-UNWRAP) and the u64 sums of vmd_eval_msd.  It IS the contract, as tests/cluster_ref.py is 1.17's: every operation below is one
fp32 operation rounded on its own, in the order the section states, so the library's sums must equal these exactly."""
import numpy as np

Q = np.float32(1048576.0)       # 2^20 quanta per square Angstrom


def cell_row(box, flags=7, tilt=(0.0, 0.0, 0.0)):
    """the nine floats behind a row's coordinates: L, fl(1 / L), the tilts - L = 1 / L = 0 on an axis that is not periodic (its flag is
    clear, or its edge is not positive)"""
    L = np.asarray(box, np.float32)
    on = np.array([(flags >> k) & 1 for k in range(3)], bool) & (L > 0)
    with np.errstate(divide="ignore"):
        inv = (np.float32(1.0) / L).astype(np.float32)
    return np.concatenate([np.where(on, L, np.float32(0)), np.where(on, inv, np.float32(0)), np.asarray(tilt, np.float32)]).astype(np.float32)


def table(coords, cells, atoms):
    """rows [F, 3 n + 9]: x[n], y[n], z[n] of `atoms` as the frames hold them (coords float32 [F, 3, N]), then cell_row of the frame's cell
    (cells: one (box, tilt, flags) for all frames, or one per frame)"""
    coords = np.asarray(coords, np.float32)
    F = coords.shape[0]
    cells = [cells] * F if isinstance(cells, tuple) else list(cells)
    atoms = np.asarray(atoms, np.int64)
    rows = np.empty((F, 3 * atoms.size + 9), np.float32)
    for f in range(F):
        box, tilt, flags = cells[f]
        rows[f, :3 * atoms.size] = coords[f][:, atoms].reshape(-1)
        rows[f, 3 * atoms.size:] = cell_row(box, flags, tilt)
    return rows


def unwrap(rows, n):
    """image counts int32 [F, 3, n] of consecutive rows: 0 in the first; from t to t + 1, under the cell of frame t + 1, a difference above
    half a cell takes the count down by one, one below minus half a cell up by one (SPEC S3's comparisons; exactly half a cell: no change)"""
    F = rows.shape[0]
    X = rows[:, :3 * n].reshape(F, 3, n)
    L = rows[:, 3 * n:3 * n + 3]
    d = X[1:] - X[:-1]                                          # fp32
    hL = (np.float32(0.5) * L[1:])[:, :, None]
    step = np.where(d > hL, -1, np.where(d < -hL, 1, 0))
    step = np.where((L[1:] > 0)[:, :, None], step, 0)
    cnt = np.zeros((F, 3, n), np.int64)
    cnt[1:] = np.cumsum(step, axis=0)
    assert np.abs(cnt).max(initial=0) < 2 ** 31
    return cnt.astype(np.int32)


def msd(rows, n, beg, end, max_lag, stride=1):
    """sums uint64 [max_lag + 1, 4] over the window [beg, end) of `rows`: per lag the quanta along x, y, z and the number of terms"""
    assert 0 <= beg < end <= rows.shape[0] and 0 <= max_lag < end - beg and stride >= 1
    W = rows[beg:end]
    F = W.shape[0]
    X = W[:, :3 * n].reshape(F, 3, n)
    L = W[:, 3 * n:3 * n + 3]
    cnt = unwrap(W, n)
    out = np.zeros((max_lag + 1, 4), np.uint64)
    for tau in range(max_lag + 1):
        t = np.arange(0, F - tau, stride)
        dn = (cnt[t + tau] - cnt[t]).astype(np.float32)
        d = (X[t + tau] - X[t]) + dn * L[t + tau][:, :, None]   # fp32: one subtraction, one product, one sum
        q = ((d * d) * Q).astype(np.uint64)                     # truncating
        out[tau, :3] = q.sum(axis=(0, 2), dtype=np.uint64)
        out[tau, 3] = t.size * n
    return out
