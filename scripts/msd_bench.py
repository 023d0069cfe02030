"""Timing of the mean-squared displacement on one GPU: 1 000 frames of the 100 002-atom synthetic water box, resident in
HBM - the position table of the 33 334 oxygens, then vmd_eval_msd over the whole window at max_lag 100 and 500, stride 1.

    python scripts/msd_bench.py [--frames 1000] [--reps 7] [--out FILE]

Three things are measured on one visit.  The query: host clock around a call that ends in a device synchronise, 1 warm-up + `reps`
calls per max_lag, and its split into the unwrap and the lags kernels from device events (the profile).  The gather: whole-range
frame_range calls (clear_data first), alternating, of count(O and within(3.5, O)) alone, of the same count with the position table next to
it, and of the table alone; what the table adds to the count is the difference of the medians, next to the gather kernel's own device time.
The term rate: column 3 of the sums (origins x atoms per lag, three axes each) over the lags kernel's time, against the LDS-read bound of
the kernel's shape derived in DESIGN 1.18.  The synthetic frames are uncorrelated, so the MSD itself means nothing here; the first two
frames of the window are checked against the NumPy restatement (tests/msd_ref.py) at this size."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import viamd_amd as V                                       # noqa: E402
from viamd_amd import synth                                 # noqa: E402
import msd_ref as R                                         # noqa: E402

ATOMS, BOX, SEED = 100002, 100.0, 2
NAME = "pos"
# the LDS-read bound: per (origin, lag, atom) a wave issues 6 ds_read_b32 for the target's x, y, z and image counts (2 LDS
# cycles each) and 3 ds_read2_b32 for the origin's (4 each): 24 LDS cycles per 64 lanes on a CU
LDS_CYCLES_PER_WAVE_TERM, CUS, CLOCK_HZ = 24.0, 256, 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--atoms", type=int, default=ATOMS, help="a smaller box at the same density (a rehearsal)")
    ap.add_argument("--lags", type=int, nargs="*", default=[100, 500])
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of the library (a rehearsal of the script's logic: its times mean nothing)")
    a = ap.parse_args()
    lib = V.VmdLib(a.lib) if a.lib else V.default_lib()
    assert lib.vmd_device_count() > 0, "needs a HIP device: there is no CPU path, and a CPU time would say nothing"
    lib.vmd_set_device(0)
    F, N = a.frames, a.atoms
    box = BOX * (N / ATOMS) ** (1.0 / 3.0)
    cell = V.make_unitcell(box)
    traj = synth.make_device_trajectory(V, SEED, N, box, F, lib=lib)
    sysm = V.MolSystem(N, unitcell=cell)
    oxy = np.arange(0, N, 3, dtype=np.int32)
    n = oxy.size

    def ir_of(within, msd):
        ir = V.ScriptIR(lib)
        if within:
            ir.add_within_count("nw", oxy, oxy, 0.0, 3.5)
        if msd:
            ir.add_msd(NAME, oxy)
        return ir
    ev_w, ev_both, ev_m = (V.ScriptEval(F, ir_of(*k)) for k in ((True, False), (True, True), (False, True)))

    def once(ev):
        ev.clear_data()
        t0 = time.perf_counter()
        assert ev.frame_range(sysm, traj, 0, F)
        return (time.perf_counter() - t0) * 1e3

    def med(x):
        return f"median {statistics.median(x):9.3f} ms   (min {min(x):.3f}, max {max(x):.3f})"

    def profiled(fn, names):
        lib.vmd_profile_reset()
        lib.vmd_profile_enable(True)
        try:
            fn()
        finally:
            lib.vmd_profile_enable(False)
        k = C.c_uint64(0)
        return {nm: lib.vmd_profile_ms(nm.encode(), C.byref(k)) for nm in names}

    evs = (ev_w, ev_both, ev_m)
    for ev in evs:                                              # warm-up: code objects, scratch, bucket capacities
        once(ev)
    t = [[] for _ in evs]
    for _ in range(a.reps):                                     # alternating
        for k, ev in enumerate(evs):
            t[k].append(once(ev))
    m = [statistics.median(x) for x in t]
    gather = profiled(lambda: once(ev_both), ("msd_gather",))["msd_gather"]
    lines = [
        f"msd (DESIGN 1.18): {F} frames of the {N}-atom synthetic water box (seed {SEED}, {box:.3f} A), resident; the position table of the "
        f"{n} oxygens, {12 * n + 36} bytes per frame, {F * (12 * n + 36) / 1e6:.1f} MB on the device and on the host; host clock around "
        f"calls that end in a device synchronise, 1 warm-up + {a.reps} calls each, alternating.",
        "---- the gather in frame_range (whole-range calls, clear_data first)",
        f"within count alone       {med(t[0])}   count(O and within(3.5, O)), the same list",
        f"within count + table     {med(t[1])}",
        f"table alone              {med(t[2])}",
        f"the table adds {m[1] - m[0]:.3f} ms to the count ({(m[1] - m[0]) / m[0]:.3f} of it), {(m[1] - m[0]) / F * 1e3:.2f} us per frame; the gather "
        f"kernel's own device time in one profiled call: {gather:.3f} ms ({F * (24 * n + 72) / gather / 1e6:.1f} GB/s read + written); the rest "
        f"is the rows' copy to the host view ({F * (12 * n + 36) / 1e6:.1f} MB) and its bookkeeping",
    ]
    ok = True
    for lag in a.lags:
        lag = min(lag, F - 1)
        ev_m.msd(NAME, 0, F, lag)                               # warm-up: the query's scratch
        tq = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = ev_m.msd(NAME, 0, F, lag)
            tq.append((time.perf_counter() - t0) * 1e3)
        split = profiled(lambda: ev_m.msd(NAME, 0, F, lag), ("msd_unwrap", "msd_lags"))
        terms = int(res.sums[:, 3].sum())
        rate = terms / (split["msd_lags"] * 1e-3)
        bound = CUS * CLOCK_HZ * 64.0 / LDS_CYCLES_PER_WAVE_TERM
        lines += [
            f"---- vmd_eval_msd, window [0, {F}), max_lag {lag}, stride 1",
            f"query          {med(tq)}",
            f"device events of one profiled call: unwrap {split['msd_unwrap']:.3f} ms, lags {split['msd_lags']:.3f} ms; the rest of the call is "
            f"the zeroing, the copy of {4 * (lag + 1)} words and the synchronise",
            f"terms (origins x atoms, summed over the lags; three axes each) {terms}: {rate:.3e} terms/s achieved in the lags kernel against "
            f"the LDS-read bound {bound:.3e} terms/s ({CUS} CUs x {CLOCK_HZ / 1e9:.1f} GHz x 64 lanes / {LDS_CYCLES_PER_WAVE_TERM:.0f} LDS cycles per "
            f"wave and term; the clock is the guide's nominal figure, not measured here): {rate / bound:.3f} of it",
        ]
        ok = ok and int(res.sums[0, 3]) == F * n and not res.sums[0, :3].any()
    rows = ev_m.property_data(NAME).msd_table[:2]
    want = R.msd(rows, n, 0, 2, 1)
    got = ev_m.msd(NAME, 0, 2, 1).sums
    same = np.array_equal(got, want)
    lines.append(f"the first two frames of the window against the NumPy restatement at this size: {'every u64 equal' if same else 'DIFFERENT SUMS'} "
                 f"(lag 1: {int(got[1, 0])}, {int(got[1, 1])}, {int(got[1, 2])} quanta over {int(got[1, 3])} terms)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    assert ok and same


if __name__ == "__main__":
    main()
