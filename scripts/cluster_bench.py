"""Timing of the cluster analysis on one GPU: 1 000 frames of the 100 002-atom synthetic water box, resident in HBM -
clusters over the 33 334 oxygens as one-atom groups, at two radii chosen from frame 0 on the CPU (one where the largest cluster holds
more than 90 % of the groups, one where it holds less than 10 %) - next to the yardstick, the cheapest walk the tree has over the same
list: count(O and within(r, O)).

    python scripts/cluster_bench.py [--frames 1000] [--reps 7] [--out FILE]

The statements are evaluated by whole-range calls (clear_data, frame_range over all frames; the call returns behind a device
synchronise), alternating, after one warm-up call each: the clusters statement as it is by default, with option cluster_skip_same 1, with
option cluster_wave_singles 0, then the yardstick; the medians (min - max), the ratio and the two A/Bs are printed.  Then one profiled
evaluation of the clusters statement gives the kernels' own times (device events around every launch group) and their shares.  A within
count leaves the walk at a lane's first hit and a union cannot, so no ratio is expected: it is written down with that said.  The routes
of the clusters statement (the cell walk, all pairs) are also checked against each other on the first frames, and frame 0's clusters
against the CPU's."""
import argparse
import ctypes as C
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import viamd_amd as V                                       # noqa: E402
from viamd_amd import _lib as L                             # noqa: E402
from viamd_amd import synth                                 # noqa: E402

ATOMS, BOX, SEED = 100002, 100.0, 2
NAMES = ("ncl", "clsz", "clmax")
KERNELS = ("cells_build", "sorted_atoms", "cluster_atoms", "cluster_brute", "cluster_finish")


def host_frame(traj, frame, n):
    """one frame of a resident trajectory on the host -> float64 [n, 3]"""
    ti = traj.interface().contents
    xyz = [np.zeros(n, np.float32) for _ in range(3)]
    hdr = L.FrameHeader()
    assert ti.load_frame(ti.inst, frame, C.byref(hdr), *[a.ctypes.data_as(L.c_float_p) for a in xyz])
    return np.stack(xyz, axis=1).astype(np.float64)


def cpu_clusters(pts, box, r):
    """the components of the points under the minimum image at d < r, in double -> (clusters, largest)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    n = pts.shape[0]
    pairs = cKDTree(np.mod(pts, box), boxsize=box).query_pairs(r, output_type="ndarray")
    m = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    ncl, lab = connected_components(m, directed=False)
    return int(ncl), int(np.bincount(lab).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--atoms", type=int, default=ATOMS, help="a smaller box at the same density (a rehearsal)")
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
    G = oxy.size
    groups = np.arange(G, dtype=np.int32)

    # the two radii, from frame 0 on the CPU: the smallest of the scan whose largest cluster holds more than 90 % of the groups, the
    # largest whose largest cluster holds less than 10 %
    pts = host_frame(traj, 0, N)[oxy]
    scan = [(r, *cpu_clusters(pts, box, r)) for r in np.round(np.arange(2.0, 6.01, 0.1), 2)]
    r_hi = min(r for r, _, big in scan if big > 0.9 * G)
    r_lo = max(r for r, _, big in scan if big < 0.1 * G)
    cpu = {r: (ncl, big) for r, ncl, big in scan}
    lines = [
        f"clusters (DESIGN 1.17): {F} frames of the {N}-atom synthetic water box (seed {SEED}, {box:.3f} A), resident; {G} oxygens as "
        f"one-atom groups; whole-range calls, host clock around a call that ends in a device synchronise, 1 warm-up + {a.reps} calls each, "
        f"alternating.  Radii from frame 0 on the CPU (double, minimum image, scan 2.0 .. 6.0 A in steps of 0.1): {r_hi} A - {cpu[r_hi][0]} "
        f"clusters, the largest {cpu[r_hi][1]} groups, {cpu[r_hi][1] / G:.3f} of all; {r_lo} A - {cpu[r_lo][0]} clusters, the largest "
        f"{cpu[r_lo][1]} groups, {cpu[r_lo][1] / G:.4f} of all.  A within count leaves the walk at a lane's first hit, a union visits every "
        f"hit: the ratio below is what that costs, not a target."]
    ok = True
    for r in (r_hi, r_lo):
        ir_c = V.ScriptIR(lib)
        ir_c.add_clusters(NAMES, oxy, groups, r)
        ir_w = V.ScriptIR(lib)
        ir_w.add_within_count("nw", oxy, oxy, 0.0, r)
        ev_c, ev_w = V.ScriptEval(F, ir_c), V.ScriptEval(F, ir_w)

        def once(ev, **opts):
            old = {k: lib.vmd_set_option(k.encode(), v) for k, v in opts.items()}
            try:
                ev.clear_data()
                t0 = time.perf_counter()
                assert ev.frame_range(sysm, traj, 0, F)
                return (time.perf_counter() - t0) * 1e3
            finally:
                for k, v in old.items():
                    lib.vmd_set_option(k.encode(), v)

        def outputs():
            return (ev_c.property_data(NAMES[1]).cluster_accumulators.copy(), ev_c.property_data(NAMES[0]).values.copy(),
                    ev_c.property_data(NAMES[2]).values.copy())

        variants = (dict(), dict(cluster_skip_same=1), dict(cluster_wave_singles=0))
        outs = []
        for v in variants:                                      # warm-up: code objects, scratch, bucket capacities
            once(ev_c, **v)
            outs.append(outputs())
        once(ev_w)
        t = [[] for _ in variants]
        tw = []
        for _ in range(a.reps):                                 # the default, the two A/B arms, the yardstick: alternating
            for k, v in enumerate(variants):
                t[k].append(once(ev_c, **v))
            tw.append(once(ev_w))
        same_ab = all(np.array_equal(x, y) for o in outs[1:] for x, y in zip(o, outs[0]))
        rec, counts, largest = outs[0]

        lib.vmd_profile_reset()
        lib.vmd_profile_enable(True)
        once(ev_c)
        lib.vmd_profile_enable(False)
        n = C.c_uint64(0)
        kern = {k: lib.vmd_profile_ms(k.encode(), C.byref(n)) for k in KERNELS}
        ksum = sum(kern.values())

        f2 = min(F, 2)                                          # the two routes on the first frames: one record
        recs = []
        for below in (0, 1 << 30):
            old = lib.vmd_set_option(b"shell_brute_below", below)
            try:
                ev = V.ScriptEval(F, ir_c)
                assert ev.frame_range(sysm, traj, 0, f2)
                recs.append((ev.property_data(NAMES[1]).cluster_accumulators.copy(), ev.property_data(NAMES[0]).values[:f2].copy(),
                             ev.property_data(NAMES[2]).values[:f2].copy()))
            finally:
                lib.vmd_set_option(b"shell_brute_below", old)
        same = all(np.array_equal(x, y) for x, y in zip(recs[0], recs[1]))
        labels, ncl0 = ev_c.cluster_labels(NAMES[0], sysm, traj, 0)

        def med(x):
            return f"median {statistics.median(x):9.3f} ms   (min {min(x):.3f}, max {max(x):.3f})"
        m = [statistics.median(x) for x in t]
        mw = statistics.median(tw)
        lines += [
            f"---- r_cut {r} A",
            f"clusters       {med(t[0])}   the default: cluster_skip_same 0, cluster_wave_singles 1",
            f"within count   {med(tw)}   count(O and within({r}, O)), the same list",
            f"ratio clusters / within count {m[0] / mw:.3f}",
            "kernels of one profiled clusters call (device events per launch group): " + ", ".join(f"{k} {v:.3f} ms" for k, v in kern.items())
            + "; shares of their sum: " + ", ".join(f"{k} {v / ksum:.3f}" for k, v in kern.items() if v),
            f"clusters per frame {counts.mean():.1f} (min {counts.min():.0f}, max {counts.max():.0f}), largest cluster per frame "
            f"{largest.mean():.1f} (min {largest.min():.0f}, max {largest.max():.0f}); record: clusters {int(rec[:-1].sum())}, of one group "
            f"{int(rec[0])}, frames {int(rec[-1])}; frame 0: {ncl0} clusters, the largest {int(np.bincount(labels).max())} (the CPU's double "
            f"scan: {cpu[r][0]}, {cpu[r][1]})",
            f"walk against all pairs on frames [0, {f2}): {'one record, bit for bit' if same else 'DIFFERENT RECORDS'}",
            f"A/B, option cluster_skip_same, alternating in this process: every hit a union {med(t[0])}, skipping repeats {med(t[1])}, "
            f"skip / every {m[1] / m[0]:.3f}",
            f"A/B, option cluster_wave_singles, alternating in this process: one add per cluster {med(t[2])}, singles per wave {med(t[0])}, "
            f"wave / each {m[0] / m[2]:.3f}; {'one record, counts and largest sizes, bit for bit, in all three' if same_ab else 'DIFFERENT OUTPUTS'}",
        ]
        inv = int((np.arange(1, G + 1, dtype=np.uint64) * rec[:-1]).sum()) == G * F
        ok = ok and same and same_ab and inv and int(rec[-1]) == F and int(rec[:-1].sum()) == int(counts.astype(np.float64).sum())
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    assert ok


if __name__ == "__main__":
    main()
