"""Timing of the hydrogen-bond analysis on one GPU: 1 000 frames of the 100 002-atom synthetic water box, resident in HBM -
66 668 donor pairs against 33 334 acceptors at r_da = 3.5 A and 150 degrees - next to the yardstick, the cheapest walk the tree has over
the same geometry: count(element('O') and within(3.5, element('O'))).

    python scripts/hbond_bench.py [--frames 1000] [--reps 7] [--out FILE]

Both statements are evaluated by whole-range calls (clear_data, frame_range over all frames; the call returns behind a device
synchronise), alternating, after one warm-up call each; the medians and the ratio are printed.  Then one profiled evaluation of the
hbonds statement gives the kernels' own times (device events around every launch group) and the share of k_sorted_atoms.  The routes of
the hbonds statement (the cell walk, all pairs) are also checked against each other on the first frames: one record, bit for bit."""
import argparse
import ctypes as C
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import viamd_amd as V                                       # noqa: E402

ATOMS, BOX, SEED, R_DA, ANGLE = 100002, 100.0, 2, 3.5, 150.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--atoms", type=int, default=ATOMS)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of the library (a rehearsal of the script's logic: its times mean nothing)")
    a = ap.parse_args()
    lib = V.VmdLib(a.lib) if a.lib else V.default_lib()
    assert lib.vmd_device_count() > 0, "needs a HIP device: there is no CPU path, and a CPU time would say nothing"
    lib.vmd_set_device(0)
    F, N = a.frames, a.atoms - a.atoms % 3
    box = BOX * (N / ATOMS) ** (1.0 / 3.0)
    cell = V.make_unitcell(box)
    traj = V.DeviceTrajectory(F, N, lib=lib)
    traj.synth(SEED, box)
    sysm = V.MolSystem(N, unitcell=cell)
    o = np.arange(0, N, 3, dtype=np.int32)
    don, hyd = np.repeat(o, 2), (np.repeat(o, 2) + np.tile([1, 2], o.size)).astype(np.int32)

    ir_h = V.ScriptIR(lib)
    ir_h.add_hbonds(("nhb", "occ"), don, hyd, o, R_DA, ANGLE)
    ir_w = V.ScriptIR(lib)
    ir_w.add_within_count("nw", o, o, 0.0, R_DA)
    ev_h, ev_w = V.ScriptEval(F, ir_h), V.ScriptEval(F, ir_w)

    def once(ev):
        ev.clear_data()
        t0 = time.perf_counter()
        assert ev.frame_range(sysm, traj, 0, F)
        return (time.perf_counter() - t0) * 1e3

    once(ev_h), once(ev_w)                                  # warm-up: code objects, scratch, bucket capacities
    th, tw = [], []
    for _ in range(a.reps):
        th.append(once(ev_h))
        tw.append(once(ev_w))
    mh, mw = statistics.median(th), statistics.median(tw)
    rec = ev_h.property_data("occ").hbond_accumulators.copy()
    counts = ev_h.property_data("nhb").values.copy()
    nw = ev_w.property_data("nw").values.copy()

    lib.vmd_profile_reset()
    lib.vmd_profile_enable(True)
    once(ev_h)
    lib.vmd_profile_enable(False)
    n = C.c_uint64(0)
    kern = {k: lib.vmd_profile_ms(k.encode(), C.byref(n)) for k in ("cells_build", "sorted_atoms", "hbond_atoms", "hbond_brute")}

    # the two routes on the first frames: one record
    f2 = min(F, 4)
    recs = []
    for below in (0, 1 << 30):
        old = lib.vmd_set_option(b"shell_brute_below", below)
        try:
            ev = V.ScriptEval(F, ir_h)
            assert ev.frame_range(sysm, traj, 0, f2)
            recs.append((ev.property_data("occ").hbond_accumulators.copy(), ev.property_data("nhb").values[:f2].copy()))
        finally:
            lib.vmd_set_option(b"shell_brute_below", old)
    same = np.array_equal(recs[0][0], recs[1][0]) and np.array_equal(recs[0][1], recs[1][1])

    npairs = don.size
    lines = [
        f"hbonds (DESIGN 1.14): {F} frames of the {N}-atom synthetic water box (seed {SEED}, {box:.3f} A), resident; {npairs} donor pairs x "
        f"{o.size} acceptors, r_da {R_DA} A, {ANGLE} degrees; whole-range calls, host clock around a call that ends in a device synchronise, "
        f"1 warm-up + {a.reps} calls each, alternating",
        f"hbonds         median {mh:9.3f} ms   (min {min(th):.3f}, max {max(th):.3f})",
        f"within count   median {mw:9.3f} ms   (min {min(tw):.3f}, max {max(tw):.3f})   count(O and within({R_DA}, O)), the same lists",
        f"ratio hbonds / within count {mh / mw:.3f}",
        "kernels of one profiled hbonds call (device events per launch group): " + ", ".join(f"{k} {v:.3f} ms" for k, v in kern.items()),
        f"share of k_sorted_atoms in the hbonds call: {kern['sorted_atoms'] / mh:.3f} of the call's median; "
        f"{kern['sorted_atoms'] / max(kern['sorted_atoms'] + kern['hbond_atoms'], 1e-9):.3f} of sorted_atoms + hbond_atoms",
        f"bonds per frame {counts.mean():.1f} (min {counts.min():.0f}, max {counts.max():.0f}); occupancy: donor rows sum "
        f"{int(rec[:npairs].sum())}, acceptor rows sum {int(rec[npairs:-1].sum())}, frames {int(rec[-1])}; oxygens with an O within "
        f"{R_DA} A per frame {nw.mean():.1f}",
        f"walk against all pairs on frames [0, {f2}): {'one record, bit for bit' if same else 'DIFFERENT RECORDS'}",
        "LDS-compacted variant of k_hbond_atoms: not built, not measured",
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    assert same and int(rec[:npairs].sum()) == int(rec[npairs:-1].sum()) == int(counts.sum()) and int(rec[-1]) == F


if __name__ == "__main__":
    main()
