"""The SDF alignment stage (k_sdf_ref_pose, k_sdf_align, k_sdf_group) on the SIMT emulator against tests/sdf_align_ref.py: weighted Kabsch
by SVD on structures whose whole form is known from their generation (tests/sdf_align_cases.py), and the reference itself against a
40-digit one.  The device side of the same cases is tests/test_sdf_align_gpu.py."""
import itertools

import numpy as np
import pytest

import sdf_align_cases as A
import sdf_align_ref as R


def test_reference_against_40_digits():
    """REF_UNITS: the fp64 reference (SVD) within REF_UNITS u of the rotation of Horn's quaternion at 40 digits - S formed exactly from
    the same fp32 inputs, the top eigenvector of N by mpmath.eigsy - over every well-conditioned (frame, structure) of the suite.  The
    kernel is not involved."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    old = mp.dps
    mp.dps = 40
    try:
        mpf = mpmath.mpf

        def whole(bt, b, k):
            A9 = [mpf(float(v)) for v in bt.boxes[b]]
            cell = [[A9[0], A9[6], A9[7]], [mpf(0), A9[1], A9[8]], [mpf(0), mpf(0), A9[2]]]
            st, n = bt.stored(b, k), bt.n[b, k] - bt.n[b, k][bt.root(k)]
            return [[mpf(float(st[a, i])) - sum(cell[i][j] * int(n[a, j]) for j in range(3)) for i in range(3)] for a in range(bt.m)]

        def centred(w, x):
            sw = sum(w)
            c = [sum(wa * xa[i] for wa, xa in zip(w, x)) / sw for i in range(3)]
            return [[xa[i] - c[i] for i in range(3)] for xa in x]

        worst, where, count = 0.0, None, 0
        for bt in A.all_batches():
            _, _, _, fits = bt.reference()
            if not (bt.kind == "well").any():
                continue
            w0 = [mpf(float(v)) for v in bt.weights(0)]
            pose = centred(w0, whole(bt, 0, 0))
            batch_worst = 0.0
            for b, k in itertools.product(range(bt.B), range(bt.K)):
                if bt.kind[b, k] != "well":
                    continue
                w = [mpf(float(v)) for v in bt.weights(k)]
                c = centred(w, whole(bt, b, k))
                S = [[sum(w[a] * c[a][i] * pose[a][j] for a in range(bt.m)) for j in range(3)] for i in range(3)]
                N = mpmath.matrix(4, 4)
                N[0, 0] = S[0][0] + S[1][1] + S[2][2]
                N[1, 1] = S[0][0] - S[1][1] - S[2][2]
                N[2, 2] = S[1][1] - S[0][0] - S[2][2]
                N[3, 3] = S[2][2] - S[0][0] - S[1][1]
                N[0, 1] = N[1, 0] = S[1][2] - S[2][1]
                N[0, 2] = N[2, 0] = S[2][0] - S[0][2]
                N[0, 3] = N[3, 0] = S[0][1] - S[1][0]
                N[1, 2] = N[2, 1] = S[0][1] + S[1][0]
                N[1, 3] = N[3, 1] = S[2][0] + S[0][2]
                N[2, 3] = N[3, 2] = S[1][2] + S[2][1]
                E, Q = mpmath.eigsy(N)
                top = max(range(4), key=lambda i: E[i])
                qw, qx, qy, qz = (Q[i, top] for i in range(4))
                nrm = mpmath.sqrt(qw * qw + qx * qx + qy * qy + qz * qz)
                qw, qx, qy, qz = qw / nrm, qx / nrm, qy / nrm, qz / nrm
                Rm = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)],
                      [2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)],
                      [2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)]]
                f = fits[b][k]
                assert f.cond <= R.COND_MAX
                dev = max(abs(float(mpf(float(f.R[i, j])) - Rm[i][j])) for i in range(3) for j in range(3))
                # the reference's own N and conditioning against the 40-digit ones
                lam = sorted((E[i] for i in range(4)), reverse=True)
                normN = mpmath.sqrt(sum(N[i, j] ** 2 for i in range(4) for j in range(4)))
                assert abs(float(normN / (lam[0] - lam[1])) / f.cond - 1.0) < 1.0e-9
                count += 1
                batch_worst = max(batch_worst, dev / f.u)
                if dev / f.u > worst:
                    worst, where = dev / f.u, (bt.name, b, k)
                assert dev <= R.REF_UNITS * f.u, f"{bt.name} ({b}, {k}): the fp64 reference is {dev / f.u:.2f} u from the 40-digit one"
            print(f"sdf_align reference, {bt.name}: worst {batch_worst:.2f} u from the 40-digit reference")
        print(f"sdf_align reference: {count} (frame, structure) pairs, worst {worst:.2f} u at {where}; REF_UNITS = {R.REF_UNITS}")
        assert count > 300
    finally:
        mp.dps = old


def test_thread_slots(emu_lib):
    A.thread_slots(emu_lib)


def test_structure_sizes(emu_lib):
    A.structure_sizes(emu_lib)


def test_masses(emu_lib):
    A.masses(emu_lib)


def test_unwrap_chain(emu_lib):
    A.unwrap_chain(emu_lib)


def test_unwrap_tree(emu_lib):
    A.unwrap_tree(emu_lib)


def test_cells(emu_lib):
    A.cells(emu_lib)


def test_strides(emu_lib):
    A.strides(emu_lib)


def test_ref_pose(emu_lib):
    A.ref_pose(emu_lib)


def test_group(emu_lib):
    A.group(emu_lib)


def test_evaluator_matrices(emu_lib):
    A.evaluator_matrices(emu_lib)


def test_wide_group_volume(emu_lib, oracle):
    A.wide_group(emu_lib, oracle)


def test_triclinic_reach_volume(emu_lib, oracle):
    A.triclinic_reach(emu_lib, oracle)
