"""Timing of the solvent-accessible surface area on one GPU: 1 000 frames of the 100 002-atom synthetic water box, resident
in HBM - Bondi radii, probe 1.4 A, 96 points - in two cases: (a) every atom measured against every atom, (b) 5 000 atoms measured against
every atom; case (a) also with ONE point per sphere, which leaves the walk and takes the point tests away.  Next to them the two
yardsticks over the same box: the hydrogen-bond statement of scripts/hbond_bench.py (66 668 donor pairs against 33 334 acceptors at
3.5 A and 150 degrees), and a within count at r_cut over the lists of each case.

    python scripts/sasa_bench.py [--frames 1000] [--reps 7] [--out FILE]

Every statement is evaluated by whole-range calls (clear_data, frame_range over all frames; the call returns behind a device
synchronise), alternating in one process, after one warm-up call each; the medians and the ratios are printed.  Then one profiled
evaluation of each sasa statement gives the kernels' own times (device events around every launch group) and their shares.  The routes of
case (b) (the cell walk, all pairs) are also checked against each other on the first frames: one record, bit for bit."""
import argparse
import ctypes as C
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import viamd_amd as V                                       # noqa: E402

ATOMS, BOX, SEED, PROBE, NPOINTS, R_DA, ANGLE = 100002, 100.0, 2, 1.4, 96, 3.5, 150.0
R_O, R_H = 1.52, 1.20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--atoms", type=int, default=ATOMS)
    ap.add_argument("--subset", type=int, default=5000)
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
    every = np.arange(N, dtype=np.int32)
    rad = np.tile(np.array([R_O, R_H, R_H], np.float32), N // 3)
    sub = np.arange(min(a.subset, N), dtype=np.int32)
    o = np.arange(0, N, 3, dtype=np.int32)
    don, hyd = np.repeat(o, 2), (np.repeat(o, 2) + np.tile([1, 2], o.size)).astype(np.int32)
    r_cut = float(2.0 * (np.float32(R_O) + np.float32(PROBE)))

    def make(fn):
        ir = V.ScriptIR(lib)
        fn(ir)
        return V.ScriptEval(F, ir)
    evs = {
        "sasa all":    make(lambda ir: ir.add_sasa(("area", "pts"), every, rad, probe=PROBE, npoints=NPOINTS)),
        "sasa subset": make(lambda ir: ir.add_sasa(("area", "pts"), every, rad, measured=sub, probe=PROBE, npoints=NPOINTS)),
        # the same statement with ONE point per sphere: the walk, the identity loads and the per-neighbour work stay, the point tests all but go
        "sasa all, 1 point": make(lambda ir: ir.add_sasa(("area", "pts"), every, rad, probe=PROBE, npoints=1)),
        "hbonds":      make(lambda ir: ir.add_hbonds(("nhb", "occ"), don, hyd, o, R_DA, ANGLE)),
        "within all":  make(lambda ir: ir.add_within_count("nw", every, every, 0.0, r_cut)),
        "within subset": make(lambda ir: ir.add_within_count("nw", sub, every, 0.0, r_cut)),
    }

    def once(ev):
        ev.clear_data()
        t0 = time.perf_counter()
        assert ev.frame_range(sysm, traj, 0, F)
        return (time.perf_counter() - t0) * 1e3

    for ev in evs.values():                                 # warm-up: code objects, scratch, bucket capacities
        once(ev)
    times = {k: [] for k in evs}
    for _ in range(a.reps):
        for k, ev in evs.items():
            times[k].append(once(ev))
    med = {k: statistics.median(v) for k, v in times.items()}

    lines = [
        f"sasa (DESIGN 1.15): {F} frames of the {N}-atom synthetic water box (seed {SEED}, {box:.3f} A), resident; Bondi radii, probe {PROBE} A, "
        f"{NPOINTS} points, r_cut {r_cut:.2f} A; whole-range calls, host clock around a call that ends in a device synchronise, 1 warm-up + "
        f"{a.reps} calls each, alternating in one process",
    ]
    for k in evs:
        lines.append(f"{k:18s} median {med[k]:10.3f} ms   (min {min(times[k]):.3f}, max {max(times[k]):.3f})")
    lines.append(f"ratios: sasa all / hbonds {med['sasa all'] / med['hbonds']:.2f}, sasa all / within all {med['sasa all'] / med['within all']:.2f}; "
                 f"sasa subset / hbonds {med['sasa subset'] / med['hbonds']:.2f}, sasa subset / within subset "
                 f"{med['sasa subset'] / med['within subset']:.2f}")

    lines.append(f"point tests against the walk: sasa all at {NPOINTS} points {med['sasa all']:.1f} ms, at 1 point {med['sasa all, 1 point']:.1f} ms - "
                 f"the walk with everything done per neighbour is {med['sasa all, 1 point'] / med['sasa all']:.3f} of the call, the point tests "
                 f"the rest")

    n = C.c_uint64(0)
    for k in ("sasa all", "sasa subset"):
        ev = evs[k]
        lib.vmd_profile_reset()
        lib.vmd_profile_enable(True)
        t = once(ev)
        lib.vmd_profile_enable(False)
        kern = {q: lib.vmd_profile_ms(q.encode(), C.byref(n)) for q in ("cells_build", "sorted_atoms", "sasa_atoms", "sasa_brute")}
        tot = max(sum(kern.values()), 1e-9)
        lines.append(f"{k}: kernels of one profiled call ({t:.3f} ms; device events per launch group): " +
                     ", ".join(f"{q} {v:.3f} ms ({v / tot:.3f})" for q, v in kern.items()))
        rec = ev.property_data("pts").sasa_accumulators.copy()
        area = ev.property_data("area").values[:F].copy()
        nmeas = rec.size - 1
        lines.append(f"{k}: mean accessible points per measured atom and frame {rec[:-1].sum() / max(int(rec[-1]), 1) / nmeas:.3f} of {NPOINTS}; "
                     f"area per frame {area.mean():.1f} A^2 (min {area.min():.1f}, max {area.max():.1f}); frames {int(rec[-1])}")
        assert int(rec[-1]) == F

    # the mean neighbours per atom, COUNTED on the first and the middle frame for a sample of 600 atoms against every atom: the pairs
    # with d < R_i + R_j, j != i, by the minimum image in float64 (a mean over 600 x 100 002 pairs does not move with the last bit of a distance), and the candidates
    # inside r_cut.  The synthetic box keeps each water's three atoms together, so an atom always has its two partners among them
    for fr in sorted({0, F // 2}):          # (the frames differ: see the spread of the areas above)
        xyz, _ = traj.download_frame(fr)
        xyz = xyz.astype(np.float64)
        R_all = (rad + np.float32(PROBE)).astype(np.float64)
        sample = np.arange(0, N, max(1, N // 600))[:600]
        nb_of = np.zeros(sample.size)
        cand = 0
        for a0 in range(0, sample.size, 100):
            i = sample[a0:a0 + 100]
            d2 = np.zeros((i.size, N))
            for k in range(3):
                dk = xyz[k][i, None] - xyz[k][None, :]
                dk -= box * np.rint(dk / box)
                d2 += dk * dk
            near = d2 < (R_all[i, None] + R_all[None, :]) ** 2
            near[np.arange(i.size), i] = False
            nb_of[a0:a0 + i.size] = near.sum(axis=1)
            cand += int((d2 < r_cut * r_cut).sum()) - i.size
        is_o = sample % 3 == 0
        lines.append(f"mean neighbours per atom, counted on frame {fr} over {sample.size} atoms ({int(is_o.sum())} O, {int((~is_o).sum())} H): "
                     f"O {nb_of[is_o].mean():.1f}, H {nb_of[~is_o].mean():.1f}, all {nb_of.mean():.1f}; candidates inside r_cut {cand / sample.size:.1f}")

    # the two routes of case (b) on the first frames: one record
    f2 = min(F, 2)
    recs = []
    for below in (0, 1 << 30):
        old = lib.vmd_set_option(b"shell_brute_below", below)
        try:
            ir = V.ScriptIR(lib)
            ir.add_sasa(("area", "pts"), every, rad, measured=sub[:1000], probe=PROBE, npoints=NPOINTS)
            ev = V.ScriptEval(F, ir)
            assert ev.frame_range(sysm, traj, 0, f2)
            recs.append((ev.property_data("pts").sasa_accumulators.copy(), ev.property_data("area").values[:f2].copy()))
        finally:
            lib.vmd_set_option(b"shell_brute_below", old)
    same = np.array_equal(recs[0][0], recs[1][0]) and np.array_equal(recs[0][1], recs[1][1])
    lines.append(f"walk against all pairs, 1 000 measured, frames [0, {f2}): {'one record, bit for bit' if same else 'DIFFERENT RECORDS'}")
    lines.append("neighbours compacted to LDS with points across lanes: not built, not measured")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    assert same


if __name__ == "__main__":
    main()
