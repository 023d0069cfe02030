"""Timing of the contact-map analysis on one GPU: 1 000 frames of the 100 002-atom synthetic water box with a blob of 2 000
ten-atom residues in front, resident in HBM - contacts over the blob's 20 000 atoms in 2 000 groups at 4.5 A, min_sep 3, the native list
taken from frame 0 - next to the yardstick, the cheapest walk the tree has over the same geometry: count(blob and within(4.5, blob)).

    python scripts/contact_bench.py [--frames 1000] [--reps 7] [--out FILE]

The statements are evaluated by whole-range calls (clear_data, frame_range over all frames; the call returns behind a device
synchronise), alternating, after one warm-up call each - the contacts statement with the direct walk kernel (option contact_lds_rows 0)
and with the LDS-row variant (1, the default), then the yardstick; the medians, the ratio and the A/B are printed.  Then one profiled
evaluation of the contacts statement per kernel gives the kernels' own times (device events around every launch group).  The routes of the contacts statement (the
cell walk, all pairs) are also checked against each other on the first frames: one record, bit for bit."""
import argparse
import ctypes as C
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import viamd_amd as V                                       # noqa: E402
from viamd_amd import synth                                 # noqa: E402

ATOMS, BOX, SEED, R_CUT, MIN_SEP, RESIDUES, PER = 100002, 100.0, 2, 4.5, 3, 2000, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--residues", type=int, default=RESIDUES)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of the library (a rehearsal of the script's logic: its times mean nothing)")
    a = ap.parse_args()
    lib = V.VmdLib(a.lib) if a.lib else V.default_lib()
    assert lib.vmd_device_count() > 0, "needs a HIP device: there is no CPU path, and a CPU time would say nothing"
    lib.vmd_set_device(0)
    F, N, n_blob = a.frames, ATOMS, a.residues * PER
    cell = V.make_unitcell(BOX)
    traj = synth.make_device_trajectory(V, SEED, N, BOX, F, n_blob=n_blob, lib=lib)
    sysm = V.MolSystem(N, unitcell=cell)
    blob = np.arange(n_blob, dtype=np.int32)
    groups = (blob // PER).astype(np.int32)
    G = a.residues

    # the native list: an IR without natives, frame 0 queried, then the IR that is timed
    ir0 = V.ScriptIR(lib)
    ir0.add_contacts(("nc", "cmap"), blob, groups, R_CUT, MIN_SEP, ngroups=G)
    native = V.ScriptEval(F, ir0).contact_pairs("nc", sysm, traj, 0)
    ir_c = V.ScriptIR(lib)
    ir_c.add_contacts(("nc", "cmap", "q"), blob, groups, R_CUT, MIN_SEP, native=native, ngroups=G)
    ir_w = V.ScriptIR(lib)
    ir_w.add_within_count("nw", blob, blob, 0.0, R_CUT)
    ev_c, ev_w = V.ScriptEval(F, ir_c), V.ScriptEval(F, ir_w)

    def once(ev):
        ev.clear_data()
        t0 = time.perf_counter()
        assert ev.frame_range(sysm, traj, 0, F)
        return (time.perf_counter() - t0) * 1e3

    def once_lds(on):
        old = lib.vmd_set_option(b"contact_lds_rows", on)
        try:
            return once(ev_c)
        finally:
            lib.vmd_set_option(b"contact_lds_rows", old)

    def outputs():
        return (ev_c.property_data("cmap").contact_accumulators.copy(), ev_c.property_data("nc").values.copy(),
                ev_c.property_data("q").values.copy())

    once_lds(0), once_lds(1), once(ev_w)                    # warm-up: code objects, scratch, bucket capacities
    tc, tl, tw = [], [], []
    for _ in range(a.reps):                                 # the direct walk, the LDS-row variant, the yardstick: alternating
        tc.append(once_lds(0))
        tl.append(once_lds(1))
        tw.append(once(ev_w))
    mc, ml, mw = statistics.median(tc), statistics.median(tl), statistics.median(tw)
    out_lds = outputs()                                     # (the last contacts call was the variant's)
    once_lds(0)
    rec, counts, q = outputs()
    same_ab = all(np.array_equal(x, y) for x, y in zip(out_lds, (rec, counts, q)))

    kern_ab = []
    for on in (0, 1):
        lib.vmd_profile_reset()
        lib.vmd_profile_enable(True)
        once_lds(on)
        lib.vmd_profile_enable(False)
        n = C.c_uint64(0)
        kern_ab.append({k: lib.vmd_profile_ms(k.encode(), C.byref(n)) for k in ("cells_build", "sorted_atoms", "contact_atoms",
                                                                                 "contact_brute", "contact_finish")})
    kern = kern_ab[1]

    # the two routes on the first frames: one record
    f2 = min(F, 4)
    recs = []
    for below in (0, 1 << 30):
        old = lib.vmd_set_option(b"shell_brute_below", below)
        try:
            ev = V.ScriptEval(F, ir_c)
            assert ev.frame_range(sysm, traj, 0, f2)
            recs.append((ev.property_data("cmap").contact_accumulators.copy(), ev.property_data("nc").values[:f2].copy(),
                         ev.property_data("q").values[:f2].copy()))
        finally:
            lib.vmd_set_option(b"shell_brute_below", old)
    same = all(np.array_equal(x, y) for x, y in zip(recs[0], recs[1]))

    P = G * (G - 1) // 2
    lines = [
        f"contacts (DESIGN 1.16): {F} frames of the {N}-atom synthetic water box (seed {SEED}, {BOX:.3f} A) with a blob of {G} residues of "
        f"{PER} atoms, resident; {n_blob} entries in {G} groups ({P} pairs, {(P + 31) // 32 * 4} bytes of bits per frame), r_cut {R_CUT} A, "
        f"min_sep {MIN_SEP}, {len(native)} native pairs from frame 0; whole-range calls, host clock around a call that ends in a device "
        f"synchronise, 1 warm-up + {a.reps} calls each, alternating",
        f"contacts       median {ml:9.3f} ms   (min {min(tl):.3f}, max {max(tl):.3f})   the default: contact_lds_rows 1",
        f"within count   median {mw:9.3f} ms   (min {min(tw):.3f}, max {max(tw):.3f})   count(blob and within({R_CUT}, blob)), the same list",
        f"ratio contacts / within count {ml / mw:.3f}",
        "kernels of one profiled contacts call (device events per launch group): " + ", ".join(f"{k} {v:.3f} ms" for k, v in kern.items()),
        f"pairs in contact per frame {counts.mean():.1f} (min {counts.min():.0f}, max {counts.max():.0f}); record: rows sum "
        f"{int(rec[:-1].sum())}, pairs ever in contact {int((rec[:-1] > 0).sum())}, frames {int(rec[-1])}; Q(0) {q[0]:.4f}, Q(last) {q[-1]:.4f}, "
        f"min Q {q.min():.4f}",
        f"walk against all pairs on frames [0, {f2}): {'one record, bit for bit' if same else 'DIFFERENT RECORDS'}",
        f"A/B, option contact_lds_rows, alternating in this process: direct walk median {mc:.3f} ms (min {min(tc):.3f}, max {max(tc):.3f}), "
        f"LDS-row variant median {ml:.3f} ms (min {min(tl):.3f}, max {max(tl):.3f}), variant / direct {ml / mc:.3f}; k_contact_atoms by "
        f"device events {kern_ab[0]['contact_atoms']:.3f} ms direct, {kern_ab[1]['contact_atoms']:.3f} ms variant; "
        f"{'one record, counts and Q, bit for bit' if same_ab else 'DIFFERENT OUTPUTS'}",
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    assert same and same_ab and int(rec[:-1].sum()) == int(counts.astype(np.float64).sum()) and int(rec[-1]) == F and q[0] == 1.0


if __name__ == "__main__":
    main()
