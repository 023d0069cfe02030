"""The descriptor cases of the vmd_ir_add_* entry points (viamd_amd/csrc/vmd_eval_ir.cpp) over the 600-atom topology of
script_cases.topology() - 30 residues of 10 atoms, then 100 waters -, written as text: one call per line, driven straight through ctypes
(viamd_amd.eval.ScriptIR checks arguments itself, so it is not used).  tests/golden/make_ir_pin.py records what the library makes of
them (tests/golden/ir_pin.json), tests/test_ir_pin.py holds the library against the record, and tests/native/ir_replay.cpp replays
dump() - the same lines with their lists written out - under sanitizers.

A line is `<ir> <entry point> <arguments>`: ir is `+` (the case's descriptor list) or `0` (NULL).  Arguments, by the letters of SPEC:
  n  a name: a word, @empty or @null                    M  names: a/b/c, or null
  L  an index list: 1,2,5..9,300..600/3 or null         c  a count: a number, or = (the length of the list before it)
  i  an integer                                         f  a float (nan and inf included)
  S  a shell: - (NULL) or sh:LIST:COUNT:rmin:rmax
  X  a shell expression: - (NULL) or `x NTERMS TRUTH K` and K shells (K = 0: terms is NULL; NTERMS may be =, meaning K)
  B  a backbone: - (NULL) or `bb NSEG N CA C NRANGES OFFSETS CLASSES` (lists or null; NSEG may be =, the length of N)
`case <id> [P]` opens a case: a fresh descriptor list; P is the population vmd_ir_geometry_atoms is asked about (1 if absent)."""
import ctypes as C

import numpy as np

from viamd_amd import _lib as L

SPEC = {"rdf": "nLcLcff", "sdf": "nLccLcf", "distance": "niLcLc", "distance_population": "nicLLLL", "angle": "nLcLcLc",
        "dihedral": "nLcLcLcLc", "angle_population": "ncLLLLLL", "dihedral_population": "ncLLLLLLLL", "shape_weights": "MLc",
        "shape_weights_population": "McLL", "rmsd": "nLc", "rmsd_population": "ncLL", "within_count": "nLcLcff",
        "rdf_shell": "nLcSLcSff", "sdf_shell": "nLccLcSf", "within_count_expr": "nLcX", "sdf_shell_expr": "nLccLcXf", "ramachandran": "MB"}

WO, W, SH0, SH1, ST = "300..600/3", "300..600", "sh:0..100:=:0:5", "sh:100..200:=:0.5:6", "0..20 2 10"
BB = "bb = 0..300/10 1..300/10 2..300/10 2 0,12,30"
# an accepted call of every entry point, {n} where the name(s) go
GOOD = {
    "rdf": f"{{n}} {WO} = {W} = 0.5 7.5",
    "sdf": f"{{n}} {ST} {WO} = 6",
    "distance": "{n} 0 0..10 = 10..20 =",
    "distance_population": "{n} 3 3 300,303,306 0,1,2,3 301,302,304,305,307,308 0,2,4,6",
    "angle": "{n} 301,302 = 300 = 0..3 =",
    "dihedral": "{n} 0 = 1 = 2 = 3,4 =",
    "angle_population": "{n} 3 0,10,20 0,1,2,3 1,11,21 0,1,2,3 2,3,12,22,23 0,2,3,5",
    "dihedral_population": "{n} 2 0,10 0,1,2 1,11 0,1,2 2,12 0,1,2 3,13,14 0,1,3",
    "shape_weights": "{n} 0..40 =",
    "shape_weights_population": "{n} 3 0..30 0,10,20,30",
    "rmsd": "{n} 0..40 =",
    "rmsd_population": "{n} 2 0..25 0,10,25",
    "within_count": f"{{n}} {WO} = 0..300 = 0 3.5",
    "rdf_shell": f"{{n}} {WO} = {SH0} {W} = - 0.5 7",
    "sdf_shell": f"{{n}} {ST} {WO} = sh:0..50:=:0:6 6",
    "within_count_expr": f"{{n}} {WO} = x = 6 2 {SH0} {SH1}",
    "sdf_shell_expr": f"{{n}} {ST} {WO} = x = 8 2 {SH0} {SH1} 6",
    "ramachandran": f"{{n}} {BB} null",
}
NAMES = {"shape_weights": 3, "shape_weights_population": 3, "ramachandran": 2}      # the entry points that define several properties
POPULATION = {"distance_population": 3, "angle_population": 3, "dihedral_population": 2, "shape_weights_population": 3, "rmsd_population": 2,
              "ramachandran": 30}

# the accepted shapes beyond GOOD, and the refusals an entry point has of its own (the common ones - ir NULL, no name, a taken name - are
# generated for every entry point by cases()); `all wrong` lines hold the order of the checks
OWN = """
case rdf_shapes
+ rdf g0 0 = 0 = 0 1
+ rdf g1 0..300 = 0..300 = 0 12
+ rdf e0 null 0 0 = 0 5
+ rdf e1 0 = 1,-2 = 0 5
+ rdf e2 0,-1 = null 0 0 5
+ rdf e3 0 = 1 = -1 5
+ rdf e4 0 = 1 = 5 5
+ rdf e5 0 = 1 = 0 nan
0 rdf @empty null 0 -1 = -1 -2
case sdf_shapes
+ sdf v0 0..10 1 10 300 = 0.25
+ sdf e0 0..10 0 10 300 = 4
+ sdf e1 0..10 1 10 null 0 4
+ sdf e2 0,-5 1 2 300 = 4
+ sdf e3 0..10 1 10 -300 = 4
+ sdf e4 0..10 1 10 300 = 0
+ sdf e5 0..10 1 10 300 = nan
0 sdf @null null 1 1 null 0 -1
case distance_kinds
+ distance d0 0 0..10 = 10..20 =
+ distance d1 1 0..10 = 10..20 =
+ distance d2 2 0..10 = 10..20 =
+ distance d3 3 0..3 = 10..12 =
+ distance e0 4 0 = 1 =
+ distance e1 -1 0 = 1 =
+ distance e2 0 null 0 1 =
+ distance e3 0 0 = 1,-1 =
+ distance e4 0 -7 = null 0
0 distance @empty 9 null 0 -1 =
case distance_population_kinds 3
+ distance_population p0 0 3 300,303,306 0,1,2,3 301,302,304,305,307,308 0,2,4,6
+ distance_population p1 1 3 300,303,306,309 0,1,2,4 301,302,304,305,307,308 0,2,4,6
+ distance_population p2 2 3 300,303,306 0,1,2,3 301,302,304,305,307 0,2,4,5
+ distance_population p3 3 3 300,303,306 0,1,2,3 301,302,304,305,307,308 0,2,4,6
+ distance_population e0 0 0 300 0,1 301 0,1
+ distance_population e1 0 1 300 null 301 0,1
+ distance_population e2 0 1 300 0,1 301 null
+ distance_population e3 5 1 300 0,1 301 0,1
+ distance_population e4 0 1 300,301 1,2 301 0,1
+ distance_population e5 0 1 300 0,1 301,302 1,2
+ distance_population e6 0 2 300,301 0,1,1 301,302 0,1,2
+ distance_population e7 0 2 300,301 0,1,2 301,302 0,2,2
+ distance_population e8 3 2 300,301,302 0,1,3 301,302 0,1,2
+ distance_population e9 3 2 300,301 0,1,2 301,302,303 0,1,3
+ distance_population e10 0 1 300,-301 0,2 301 0,1
+ distance_population e11 0 1 300 0,1 -1 0,1
+ distance_population e12 0 1 null 0,1 301 0,1
0 distance_population @empty 9 0 null null null null
+ distance_population e13 9 1 null 5,2 null 3,1
case angle_shapes
+ angle a0 0 = 1 = 2 =
+ angle e0 null 2147483648 1 = 2 =
+ angle e1 0 = null 4294967296 2 =
+ angle e2 null 0 1 = 2 =
+ angle e3 0 = 1 = null 0
+ angle e4 0 = 1,-1 = 2 =
0 angle @empty null 0 null 0 null 9999999999
0 angle @empty null 0 null 0 null 0
case dihedral_shapes
+ dihedral t0 0,1 = 2,3 = 4,5 = 6,7,8 =
+ dihedral e0 0 = 1 = 2 = null 2147483648
+ dihedral e1 0 = 1 = 2 = null 0
+ dihedral e2 0 = 1 = -2 = 3 =
0 dihedral @null null 0 null 0 null 0 null 0
case angle_population_shapes 2
+ angle_population a0 2 0,10 0,1,2 1,11 0,1,2 2,12,13 0,1,3
+ angle_population e0 0 0 0,1 1 0,1 2 0,1
+ angle_population e1 1 0 0,1 1 null 2 0,1
+ angle_population e2 1 0 0,1 1 0,1 2,3 1,2
+ angle_population e3 2 0,1 0,1,2 1,2 0,1,2 2,3 0,1,1
+ angle_population e4 1 0 0,1 -1 0,1 2 0,1
+ angle_population e5 1 null 0,1 1 0,1 2 0,1
0 angle_population @empty 0 null null null null null null
+ angle_population e6 1 null null -1 3,1 null null
case dihedral_population_shapes 2
+ dihedral_population t0 2 0,10 0,1,2 1,11 0,1,2 2,12 0,1,2 3,13 0,1,2
+ dihedral_population e0 0 0 0,1 1 0,1 2 0,1 3 0,1
+ dihedral_population e1 1 0 0,1 1 0,1 2 0,1 3 null
+ dihedral_population e2 1 0 0,1 1 0,1 2 0,1 3,4 2,3
+ dihedral_population e3 1 0 0,1 1 0,1 2 0,1 3 0,0
+ dihedral_population e4 1 0 0,1 1 0,1 2 0,1 -3 0,1
0 dihedral_population @empty 0 null null null null null null null null
case shape_shapes
+ shape_weights l0/p0/i0 5 =
+ shape_weights x/y/x 0..10 =
+ shape_weights x/@empty/z 0..10 =
+ shape_weights x/@null/z 0..10 =
+ shape_weights null 0..10 =
+ shape_weights a/b/c null 2147483648
+ shape_weights a/b/c null 0
+ shape_weights a/b/c 0,-1 =
0 shape_weights null null 4294967296
0 shape_weights null null 0
+ shape_weights null null 0
case shape_population_shapes 2
+ shape_weights_population l0/p0/i0 2 0..25 0,10,25
+ shape_weights_population a/b/c 0 0 0,1
+ shape_weights_population a/b/c 1 0 null
+ shape_weights_population a/b/c 1 0,1 1,2
+ shape_weights_population a/b/c 2 0,1 0,1,1
+ shape_weights_population a/b/c 1 -1 0,1
+ shape_weights_population a/b/c 1 null 0,1
+ shape_weights_population a/a/c 0 null null
0 shape_weights_population null 0 null null
+ shape_weights_population null 0 null null
case rmsd_shapes
+ rmsd m0 7 =
+ rmsd e0 null 2147483648
+ rmsd e1 null 0
+ rmsd e2 0,1,-1 =
0 rmsd @empty null 4294967296
0 rmsd @empty null 0
case rmsd_population_shapes 3
+ rmsd_population m0 3 0..30 0,10,20,30
+ rmsd_population e0 0 0 0,1
+ rmsd_population e1 1 0 null
+ rmsd_population e2 1 0,1 1,2
+ rmsd_population e3 2 0,1 0,1,1
+ rmsd_population e4 1 -1 0,1
+ rmsd_population e5 1 null 0,1
0 rmsd_population @empty 0 null null
+ rmsd_population @empty 0 null null
case within_count_shapes
+ within_count n0 300 = 0 = 0 1
+ within_count n1 300..600 = 300..600/3 = 2.5 3.5
+ within_count e0 null 0 0 = 0 3
+ within_count e1 300 = null 0 0 3
+ within_count e2 300,-1 = 0 = 0 3
+ within_count e3 300 = -1 = 0 3
+ within_count e4 300 = 0 = nan 3
+ within_count e5 300 = 0 = 0 inf
+ within_count e6 300 = 0 = -1 3
+ within_count e7 300 = 0 = 3 3
0 within_count @empty null 0 null 0 nan nan
case rdf_shell_shapes
+ rdf_shell g0 300..600/3 = - 300..600 = - 0.5 7
+ rdf_shell g1 300..600/3 = sh:0..100:=:0:5 300..600 = - 0.5 7
+ rdf_shell g2 300..600/3 = - 300..600 = sh:0..50:=:1:4 0 7
+ rdf_shell g3 300..600/3 = sh:0..100:=:0:5 300..600 = sh:100..300:=:0.5:9 0 7
+ rdf_shell e0 null 0 sh:0:=:0:5 300 = - 0 7
+ rdf_shell e1 300 = sh:0:=:0:5 300,-1 = - 0 7
+ rdf_shell e2 300 = sh:0:=:0:5 300 = - 7 7
+ rdf_shell e3 300 = sh:null:0:0:5 300 = - 0 7
+ rdf_shell e4 300 = - 300 = sh:0,-1:=:0:5 0 7
+ rdf_shell e5 300 = sh:0:=:nan:5 300 = - 0 7
+ rdf_shell e6 300 = - 300 = sh:0:=:5:5 0 7
+ rdf_shell e7 300 = sh:0:=:0:inf 300 = sh:null:0:0:1 0 7
+ rdf_shell e8 300 = - null 0 - 0 7
0 rdf_shell @empty null 0 sh:null:0:nan:nan -1 = sh:-1:=:3:1 -1 -2
0 rdf_shell @empty null 0 - -1 = - -1 -2
case sdf_shell_shapes
+ sdf_shell v0 0..20 2 10 300..600/3 = - 6
+ sdf_shell v1 0..20 2 10 300..600/3 = sh:0..50:=:0.5:6 6
+ sdf_shell e0 0..20 0 10 300 = sh:0:=:0:5 6
+ sdf_shell e1 0..20 2 10 null 0 sh:0:=:0:5 6
+ sdf_shell e2 0..20 2 10 300 = sh:0:=:0:5 0
+ sdf_shell e3 0..20 2 10 300 = sh:null:0:0:5 6
+ sdf_shell e4 0..20 2 10 300 = sh:-1:=:0:5 6
+ sdf_shell e5 0..20 2 10 300 = sh:0:=:-1:5 6
+ sdf_shell e6 0..20 2 10 300 = sh:0:=:0:inf 6
0 sdf_shell @empty null 0 0 null 0 sh:null:0:nan:nan -1
0 sdf_shell @empty null 0 0 null 0 - -1
case within_count_expr_shapes
+ within_count_expr n1 300..600/3 = x = 2 1 sh:0..100:=:0:5
+ within_count_expr n1n 300..600/3 = x = 1 1 sh:0..100:=:0:5
+ within_count_expr n2 300..600/3 = x = 6 2 sh:0..100:=:0:5 sh:100..200:=:0.5:6
+ within_count_expr n3 300..600/3 = x = 128 3 sh:0..100:=:0:5 sh:100..200:=:0.5:6 sh:300..600/3:=:2:3
+ within_count_expr n4 300..600/3 = x = 32768 4 sh:0..100:=:0:5 sh:100..200:=:0.5:6 sh:300..600/3:=:2:3 sh:7:=:0:9
+ within_count_expr n1t 300..600/3 = x = 3 1 sh:0..100:=:0:5
+ within_count_expr e0 300 = -
+ within_count_expr e1 300 = x 0 0 0
+ within_count_expr e2 300 = x 5 0 1 sh:0:=:0:5
+ within_count_expr e3 300 = x 2 0 0
+ within_count_expr e4 300 = x = 4 1 sh:0:=:0:5
+ within_count_expr e5 300 = x = 16 2 sh:0:=:0:5 sh:1:=:0:5
+ within_count_expr e6 300 = x = 2 1 sh:null:0:0:5
+ within_count_expr e7 300 = x = 6 2 sh:0:=:0:5 sh:-1:=:0:5
+ within_count_expr e8 300 = x = 6 2 sh:0:=:0:5 sh:1:=:nan:5
+ within_count_expr e9 300 = x = 6 2 sh:0:=:5:5 sh:1:=:0:5
+ within_count_expr e10 null 0 x = 2 1 sh:0:=:0:5
+ within_count_expr e11 -300 = x = 2 1 sh:0:=:0:5
+ within_count_expr n1 300..600/3 = x = 2 1 sh:0..100:=:0:5
0 within_count_expr @empty null 0 -
+ within_count_expr @empty null 0 -
+ within_count_expr e12 null 0 x 9 255 0
case sdf_shell_expr_shapes
+ sdf_shell_expr v1 0..20 2 10 300..600/3 = x = 2 1 sh:0..50:=:0:6 6
+ sdf_shell_expr v1n 0..20 2 10 300..600/3 = x = 1 1 sh:0..50:=:0:6 6
+ sdf_shell_expr v2 0..20 2 10 300..600/3 = x = 8 2 sh:0..100:=:0:5 sh:100..200:=:0.5:6 6
+ sdf_shell_expr v3 0..20 2 10 300..600/3 = x = 23 3 sh:0..100:=:0:5 sh:100..200:=:0.5:6 sh:300..600/3:=:2:3 4.5
+ sdf_shell_expr v4 0..10 1 10 300..600/3 = x = 65535 4 sh:0..100:=:0:5 sh:100..200:=:0.5:6 sh:300..600/3:=:2:3 sh:7:=:0:9 6
+ sdf_shell_expr e0 0..20 0 10 300 = x = 2 1 sh:0:=:0:5 6
+ sdf_shell_expr e1 0..20 2 10 null 0 x = 2 1 sh:0:=:0:5 6
+ sdf_shell_expr e2 0..20 2 10 300 = x = 2 1 sh:0:=:0:5 0
+ sdf_shell_expr e3 0..20 2 10 300 = - 6
+ sdf_shell_expr e4 0..20 2 10 300 = x 0 0 0 6
+ sdf_shell_expr e5 0..20 2 10 300 = x 5 0 1 sh:0:=:0:5 6
+ sdf_shell_expr e6 0..20 2 10 300 = x = 4 1 sh:0:=:0:5 6
+ sdf_shell_expr e7 0..20 2 10 300 = x = 6 2 sh:0:=:0:5 sh:null:0:0:5 6
+ sdf_shell_expr e8 0..20 2 10 300 = x = 6 2 sh:0:=:0:5 sh:-4:=:0:5 6
+ sdf_shell_expr e9 0..20 2 10 300 = x = 6 2 sh:0:=:0:inf sh:1:=:0:5 6
+ sdf_shell_expr v1 0..20 2 10 300..600/3 = x = 2 1 sh:0..50:=:0:6 6
0 sdf_shell_expr @empty null 0 0 null 0 - -1
+ sdf_shell_expr @empty null 0 0 null 0 - -1
+ sdf_shell_expr e10 null 0 0 null 0 - -1
+ sdf_shell_expr e11 0 1 1 null 0 - -1
+ sdf_shell_expr e12 0 1 1 300 = x 9 255 0 -1
case ramachandran_shapes 30
+ ramachandran t0/m0 bb = 0..300/10 1..300/10 2..300/10 3 0,1,12,30 0,1,2,3,255,0,1,2,3,255,0,1,2,3,255,0,1,2,3,255,0,1,2,3,255,0,1,2,3,255
+ ramachandran t1/m1 bb = 0 1 2 1 0,1 null
+ ramachandran null bb = 0 1 2 1 0,1 null
+ ramachandran a/b -
+ ramachandran a/@empty bb = 0 1 2 1 0,1 null
+ ramachandran a/a bb = 0 1 2 1 0,1 null
+ ramachandran a/t0 bb = 0 1 2 1 0,1 null
+ ramachandran a/b bb 0 0 1 2 1 0,1 null
+ ramachandran a/b bb 1073741824 0 1 2 1 0,1 null
+ ramachandran a/b bb 1 null 1 2 1 0,1 null
+ ramachandran a/b bb 1 0 null 2 1 0,1 null
+ ramachandran a/b bb 1 0 1 null 1 0,1 null
+ ramachandran a/b bb = -1 1 2 1 0,1 null
+ ramachandran a/b bb = 0 -1 2 1 0,1 null
+ ramachandran a/b bb = 0 1 -2 1 0,1 null
+ ramachandran a/b bb = 0 1 2 1 null null
+ ramachandran a/b bb = 0 1 2 0 0,1 null
+ ramachandran a/b bb = 0 1 2 1 1,2 null
+ ramachandran a/b bb = 0,3 1,4 2,5 2 0,0,2 null
+ ramachandran a/b bb = 0,3 1,4 2,5 1 0,1 null
+ ramachandran a/b bb = 0,3 1,4 2,5 1 0,2 0,7
0 ramachandran null -
+ ramachandran null -
+ ramachandran @empty/@empty bb 0 null null null 0 null null
+ ramachandran a/a bb 0 null null null 0 null null
+ ramachandran a/b bb 1073741824 null null null 0 null null
+ ramachandran a/b bb 1 -1 null null 0 null 9
+ ramachandran a/b bb 1 -1 -1 -1 0 null 9
+ ramachandran a/b bb 1 0 1 2 0 null 9
+ ramachandran a/b bb 1 0 1 2 2 1,1,5 9
"""


def names_of(entry, k=0):
    """the k-th set of fresh names for an entry point: one word, or a/b/c"""
    n = NAMES.get(entry, 1)
    return "/".join(f"{entry[0]}{k}{'abc'[j]}" for j in range(n)) if n > 1 else f"{entry[0]}{k}"


def cases():
    """-> [(id, P, [line, ...])]: per entry point the accepted call of GOOD, the same name again (taken), the calls without a descriptor
    list or a name; then the cases of OWN"""
    out = []
    for entry, good in GOOD.items():
        first, second = names_of(entry, 0), names_of(entry, 1)
        lines = [f"+ {entry} {good.format(n=first)}", f"+ {entry} {good.format(n=second)}", f"+ {entry} {good.format(n=first)}",
                 f"0 {entry} {good.format(n=names_of(entry, 2))}"]
        if entry in NAMES:      # a taken name in the last place, the same name twice
            taken = second.split("/")[-1]
            lines.append(f"+ {entry} {good.format(n='/'.join(['q0', 'q1', taken][-NAMES[entry]:]))}")
            lines.append(f"+ {entry} {good.format(n='/'.join(['r0', 'r1', 'r1'][-NAMES[entry]:]))}")
            lines.append(f"+ {entry} {good.format(n='/'.join(['@empty', 'r1', 'r2'][-NAMES[entry]:]))}")
        else:
            lines += [f"+ {entry} {good.format(n='@empty')}", f"+ {entry} {good.format(n='@null')}"]
        out.append((entry, POPULATION.get(entry, 1), lines))
    cur = None
    for line in OWN.strip().splitlines():
        if line.startswith("case "):
            w = line.split()
            cur = (w[1], int(w[2]) if len(w) > 2 else 1, [])
            out.append(cur)
        else:
            cur[2].append(line)
    return out


def expand(token):
    """an index list token -> [int] or None"""
    if token == "null":
        return None
    out = []
    for part in token.split(","):
        if ".." in part:
            rng, _, step = part.partition("/")
            a, b = rng.split("..")
            out += range(int(a), int(b), int(step or 1))
        else:
            out.append(int(part))
    return out


def _plain_shell(token):
    if token == "-":
        return token
    _, lst, cnt, rmin, rmax = token.split(":")
    v = expand(lst)
    return f"sh:{'null' if v is None else ','.join(map(str, v))}:{cnt}:{rmin}:{rmax}"


def dump():
    """the cases as the text tests/native/ir_replay.cpp reads: the same lines, every list written out"""
    text = []
    for cid, P, lines in cases():
        text.append(f"case {cid} {P}")
        for line in lines:
            words = line.split()
            for k, w in enumerate(words[2:], 2):
                if w.startswith("sh:"):
                    words[k] = _plain_shell(w)
                elif ".." in w:
                    words[k] = ",".join(map(str, expand(w)))
            text.append(" ".join(words))
    return "\n".join(text) + "\n"


# ---- one line through ctypes ------------------------------------------------------------------------------------------------------------------

class _Args:
    def __init__(self, words):
        self.words, self.k, self.keep, self.last = words, 0, [], 0

    def word(self):
        self.k += 1
        return self.words[self.k - 1]

    def name(self, w=None):
        w = self.word() if w is None else w
        return None if w == "@null" else b"" if w == "@empty" else w.encode()

    def names(self):
        w = self.word()
        if w == "null":
            return None
        parts = [self.name(x) for x in w.split("/")]
        return (C.c_char_p * len(parts))(*parts)

    def array(self, token, dtype=np.int32):
        v = expand(token)
        self.last = 0 if v is None else len(v)
        if v is None:
            return None
        a = np.array(v, np.int64).astype(dtype)
        self.keep.append(a)
        return a.ctypes.data_as(C.POINTER(C.c_uint32 if dtype == np.uint32 else C.c_uint8 if dtype == np.uint8 else C.c_int32))

    def count(self, w=None):
        w = self.word() if w is None else w
        return self.last if w == "=" else int(w)

    def shell_struct(self, token):
        _, lst, cnt, rmin, rmax = token.split(":")
        p = self.array(lst)
        return L.ShellC(p, self.count(cnt), float(rmin), float(rmax))

    def shell(self):
        w = self.word()
        if w == "-":
            return None
        s = self.shell_struct(w)
        self.keep.append(s)
        return C.byref(s)

    def expr(self):
        if self.word() == "-":
            return None
        nterms, truth, k = self.word(), int(self.word()), int(self.word())
        arr = (L.ShellC * max(k, 1))(*[self.shell_struct(self.word()) for _ in range(k)])
        x = L.ShellExprC(C.cast(arr, C.POINTER(L.ShellC)) if k else None, k if nterms == "=" else int(nterms), truth)
        self.keep += [arr, x]
        return C.byref(x)

    def backbone(self):
        if self.word() == "-":
            return None
        nseg = self.word()
        n = self.array(self.word())
        nseg = self.count(nseg)
        ca, c = self.array(self.word()), self.array(self.word())
        nranges = int(self.word())
        off, cls = self.array(self.word(), np.uint32), self.array(self.word(), np.uint8)
        bb = L.BackboneC(nseg, n, ca, c, nranges, off, cls)
        self.keep.append(bb)
        return C.byref(bb)


def call(lib, ir, line):
    """one line -> (accepted?, the entry point)"""
    words = line.split()
    a = _Args(words[2:])
    read = {"n": a.name, "M": a.names, "L": lambda: a.array(a.word()), "c": a.count, "i": lambda: int(a.word()), "f": lambda: float(a.word()),
            "S": a.shell, "X": a.expr, "B": a.backbone}
    args = [read[ch]() for ch in SPEC[words[1]]]
    assert a.k == len(a.words), line
    ok = getattr(lib, "vmd_ir_add_" + words[1])(ir if words[0] == "+" else None, *args)
    return bool(ok), words[1]


def atoms(lib, ir, name, context, cap=None):
    """vmd_ir_geometry_atoms -> [count, the atoms written]; cap None: a buffer of 4096 (ample), else `cap` entries, the rest must stay"""
    buf = np.full(4096, -7, np.int32)
    n = int(lib.vmd_ir_geometry_atoms(ir, name, context, buf.ctypes.data_as(L.c_int32_p), 4096 if cap is None else cap))
    wrote = min(n, 4096 if cap is None else cap)
    assert (buf[wrote:] == -7).all(), (name, context, cap)
    return [n, buf[:wrote].tolist()]


def eval_facts(lib, ir, names):
    """what vmd_eval_create over 3 frames sets up per property, under both settings of spec_angle_radians"""
    out = []
    for radians in (0, 1):
        old = lib.vmd_set_option(b"spec_angle_radians", radians)
        try:
            ev = lib.vmd_eval_create(3, ir)
            assert ev, lib.last_error()
            facts = {}
            for n in names:
                d = lib.vmd_eval_property_data(ev, n.encode()).contents
                facts[n] = dict(dim=list(d.dim), unit_str=[(u or b"").decode() for u in d.unit_str], min_range=list(d.min_range),
                                max_range=list(d.max_range), num_values=int(d.num_values), aggregate=bool(d.aggregate))
            lib.vmd_eval_free(ev)
        finally:
            lib.vmd_set_option(b"spec_angle_radians", old)
        out.append(facts)
    return out


def outcome(lib, P, lines, with_eval=True):
    """the whole outcome of a case, as JSON-able data, and the entry points its accepted calls reached"""
    ir = lib.vmd_ir_create()
    reached, calls = set(), []
    try:
        for line in lines:
            lib.vmd_clear_last_error()
            ok, entry = call(lib, ir, line)
            calls.append("ok" if ok else lib.last_error())
            if ok:
                reached.add(entry)
        count = int(lib.vmd_ir_property_count(ir))
        p = lib.vmd_ir_property_names(ir)
        names = [p[i].decode() for i in range(count)]
        out = dict(calls=calls, fingerprint=str(int(lib.vmd_ir_fingerprint(ir))), names=names,
                   flags=[int(lib.vmd_ir_property_flags(ir, n.encode())) for n in names], work=int(lib.vmd_ir_work_per_frame(ir)), atoms={})
        for n in names:
            full = {str(c): atoms(lib, ir, n.encode(), c) for c in (-1, 0, P - 1, P)}
            short = {str(c): atoms(lib, ir, n.encode(), c, cap=full[str(c)][0] // 2) for c in (-1, 0)}
            out["atoms"][n] = [full, short]
        if with_eval and names:
            out["eval"] = eval_facts(lib, ir, names)
        return out, reached
    finally:
        lib.vmd_ir_free(ir)
