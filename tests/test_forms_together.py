"""Every property form in one eval (the dispatch, not the arithmetic): rdf, rdf over a shell, sdf, sdf over a shell, sdf over a two-term
expression, distance, a distance_pair population, an angle, a dihedral population, a shape_weights population, rmsd, a within count, a
within-expression count and a Ramachandran table with its map stand in one script over the 600-atom topology of script_cases.topology(),
5 periodic orthorhombic frames, batch_frames = 2 (batches of 2, 2 and 1).  Every property's values, counts, weights64 and aggregate are,
bit for bit, those of an eval that holds that statement alone - and the single evals are what the per-form tests hold to their
references.  The shape triple and the Ramachandran pair stand neither first nor last."""
import numpy as np
import pytest

import viamd_amd as V
from viamd_amd import _lib as L

import script_cases as SC
from test_within import evaluate, options

FRAMES, BOX = 5, (31.0, 29.0, 33.0)
BLOB = np.arange(300, dtype=np.int32)
WO, WH = np.arange(300, 600, 3, dtype=np.int32), np.setdiff1d(np.arange(300, 600), np.arange(300, 600, 3)).astype(np.int32)
STRUCTS = np.arange(20, dtype=np.int32).reshape(2, 10)
RES = np.arange(30, dtype=np.int32)
TERMS = [(BLOB[:100], 0.0, 5.0), (BLOB[100:200], 0.5, 6.0)]

# (names, how the statement is added)
STATEMENTS = (
    (("g",), lambda ir: ir.add_rdf("g", WO, WO, 8.0)),
    (("gs",), lambda ir: ir.add_rdf_shell("gs", WO, WH, (0.5, 7.0), ref_shell=(BLOB[:100], 0.0, 5.0))),
    (("ang",), lambda ir: ir.add_angle("ang", [301, 302], [300], [0, 1, 2])),
    (("lin", "plan", "iso"), lambda ir: ir.add_shape_weights_population(("lin", "plan", "iso"), [np.arange(10 * r, 10 * r + 10) for r in range(4)])),
    (("v",), lambda ir: ir.add_sdf("v", STRUCTS, WO, 6.0)),
    (("vs",), lambda ir: ir.add_sdf_shell("vs", STRUCTS, WO, 6.0, target_shell=(BLOB[:50], 0.0, 6.0))),
    (("ve",), lambda ir: ir.add_sdf_shell_expr("ve", STRUCTS, WO, 6.0, TERMS, 0b1000)),
    (("d",), lambda ir: ir.add_distance("d", BLOB[:10], BLOB[10:20])),
    (("table", "map"), lambda ir: ir.add_ramachandran(("table", "map"), 10 * RES, 10 * RES + 1, 10 * RES + 2, [0, 12, 30],
                                                       np.array([0, 1, 2, 3, 255] * 6, np.uint8))),
    (("dp",), lambda ir: ir.add_distance_population("dp", [[300 + 3 * w] for w in range(5)], [[301 + 3 * w, 302 + 3 * w] for w in range(5)],
                                                    kind=L.DIST_PAIR)),
    (("dih",), lambda ir: ir.add_dihedral_population("dih", *[[[10 * r + k] for r in range(4)] for k in range(4)])),
    (("m",), lambda ir: ir.add_rmsd("m", BLOB[:40])),
    (("nw",), lambda ir: ir.add_within_count("nw", WO, BLOB, 0.0, 3.5)),
    (("ne",), lambda ir: ir.add_within_count_expr("ne", WO, TERMS, 0b0110)),
)


def coordinates():
    """600 atoms placed uniformly in the cell, every atom jittered by 0.4 A from frame to frame: float32 [5, 3, 600]"""
    assert SC.topology().elements.size == 600
    rng = np.random.default_rng(600)
    base = rng.uniform(0.0, 1.0, (600, 3)) * np.asarray(BOX)
    xyz = np.stack([np.mod(base + rng.normal(0.0, 0.4, base.shape) * f, BOX) for f in range(FRAMES)])
    return np.ascontiguousarray(xyz.astype(np.float32).transpose(0, 2, 1))


def record(ev, name):
    """what the host reads of a property, as bytes: values, counts, weights64, the aggregate's arrays"""
    pd = ev.property_data(name)
    out = {"dim": tuple(pd.dim), "values": pd.values.tobytes()}
    out["counts"] = None if pd.counts is None else pd.counts.tobytes()
    out["weights64"] = None if pd.weights64 is None else pd.weights64.tobytes()
    agg = pd.aggregate
    out["aggregate"] = None if agg is None else {k: np.asarray(v).tobytes() for k, v in agg.items()}
    return out


def together_and_alone(lib, device):
    coords = coordinates()
    with options(lib, batch_frames=2):
        ir = V.ScriptIR(lib)
        for _, add in STATEMENTS:
            add(ir)
        assert ir.property_names() == [n for names, _ in STATEMENTS for n in names]
        ev = evaluate(lib, ir, coords, BOX, device=device)
        together = {n: record(ev, n) for n in ir.property_names()}
        for names, add in STATEMENTS:
            one = V.ScriptIR(lib)
            add(one)
            ev1 = evaluate(lib, one, coords, BOX, device=device)
            for n in names:
                alone = record(ev1, n)
                assert alone["values"] != bytes(len(alone["values"])), f"{n}: the single eval is all zeros, the case holds nothing"
                for key in ("dim", "values", "counts", "weights64", "aggregate"):
                    assert together[n][key] == alone[key], f"{n}: {key} differs between the whole script and the statement alone"
        dist = {n for n in together if together[n]["weights64"] is not None}
        assert dist == {"g", "gs"}
        assert {n for n in together if together[n]["counts"] is not None} == {"g", "gs", "v", "vs", "ve", "map"}
        assert {n for n in together if together[n]["aggregate"] is not None} == {"lin", "plan", "iso", "dp", "dih"}


def test_every_form_in_one_eval_on_the_emulator(emu_lib):
    together_and_alone(emu_lib, False)


@pytest.mark.gpu
def test_every_form_in_one_eval_on_the_device(gpu_lib):
    together_and_alone(gpu_lib, True)
