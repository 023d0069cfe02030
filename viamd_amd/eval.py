"""Host-side mirror of the md_script evaluation surface VIAMD uses, over the C ABI.

Names follow the reference: ScriptIR ~ md_script_ir_t, ScriptEval ~ md_script_eval_t (create / clear_data /
frame_range / interrupt / property_data / frame_mask), see /root/reference/src/main.cpp:951-1039, :1286, :1513.
Everything here is plumbing: the arithmetic runs in the HIP kernels behind libviamd_amd.so.
"""
import ctypes as C
import math

import numpy as np

from . import _lib as L


def _idx(a):
    a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    return a, a.ctypes.data_as(L.c_int32_p)


def make_unitcell(box, flags=L.PBC_ALL, tilt=(0.0, 0.0, 0.0)):
    """box: None (no cell), scalar (cubic) or (x,y,z); tilt = (xy, xz, yz) of a triclinic cell
    (basis a=(x,0,0), b=(xy,y,0), c=(xz,yz,z), as VIAMD reads md_unitcell_t, src/viamd.cpp:1837-1843)."""
    if box is None:
        return L.Unitcell(0, 0, 0, 0, 0, 0, 0)
    if np.isscalar(box):
        box = (box, box, box)
    return L.Unitcell(float(box[0]), float(box[1]), float(box[2]), float(tilt[0]), float(tilt[1]), float(tilt[2]), flags)


class VmdError(RuntimeError):
    pass


class MolSystem:
    """The slice of md_system_t the evaluator reads: atom count, masses, unit cell (src/main.cpp:642)."""

    def __init__(self, num_atoms, mass=None, unitcell=None, bonds=None):
        """bonds: int32 [nbonds, 2] atom index pairs (md_system_t::bond) or None: sdf() structures are then made whole along
        their index order instead of along the bond graph."""
        self.num_atoms = int(num_atoms)
        self.mass = np.ascontiguousarray(mass if mass is not None else np.ones(num_atoms), dtype=np.float32)
        assert self.mass.size == self.num_atoms
        self.c = L.System()
        self.c.atom_count = self.num_atoms
        self.c.mass = self.mass.ctypes.data_as(L.c_float_p)
        self.c.unitcell = unitcell if unitcell is not None else make_unitcell(None)
        self.bonds = None
        if bonds is not None and len(bonds):
            self.bonds = np.ascontiguousarray(bonds, dtype=np.int32).reshape(-1, 2)
            self.c.bonds = self.bonds.ctypes.data_as(C.POINTER(C.c_int32))
            self.c.bond_count = self.bonds.shape[0]


class ScriptIR:
    """Property descriptors (md_script_ir_t stand-in)."""

    def __init__(self, lib=None):
        self.lib = lib or L.default_lib()
        self.h = self.lib.vmd_ir_create()
        if not self.h:
            raise VmdError("vmd_ir_create failed")

    def close(self):
        if self.h:
            self.lib.vmd_ir_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, ok):
        if not ok:
            raise VmdError(self.lib.last_error())

    def add_rdf(self, name, ref, target, cutoff, rmin=0.0):
        """`name = rdf(ref, target, cutoff)` (src/main.cpp:528); cutoff may be (rmin, rmax)."""
        if not np.isscalar(cutoff):
            rmin, cutoff = cutoff
        r, rp = _idx(ref)
        t, tp = _idx(target)
        self._check(self.lib.vmd_ir_add_rdf(self.h, name.encode(), rp, r.size, tp, t.size, float(rmin), float(cutoff)))

    def add_rdf_shell(self, name, ref, target, cutoff, rmin=0.0, ref_shell=None, target_shell=None):
        """`name = rdf(ref and within(a:b, R), target, cutoff)`: either side may be a shell, given as (R, r_min, r_max) - per
        frame, the atoms of that side's list with some atom of R at r_min <= d < r_max.  Both None: add_rdf."""
        if not np.isscalar(cutoff):
            rmin, cutoff = cutoff
        import ctypes as C
        r, rp = _idx(ref)
        t, tp = _idx(target)
        keep, ptrs = [], []
        for sh in (ref_shell, target_shell):
            if sh is None:
                ptrs.append(None)
                continue
            x, xp = _idx(sh[0])
            c = L.ShellC(xp, x.size, float(sh[1]), float(sh[2]))
            keep.append((x, c))
            ptrs.append(C.byref(c))
        self._check(self.lib.vmd_ir_add_rdf_shell(self.h, name.encode(), rp, r.size, ptrs[0], tp, t.size, ptrs[1], float(rmin), float(cutoff)))

    def add_sdf(self, name, structures, target, cutoff):
        """`name = sdf(structures, target, cutoff)`; structures: [K, m] atom indices."""
        s = np.ascontiguousarray(structures, dtype=np.int32)
        if s.ndim != 2:
            raise ValueError("structures must be a [K, m] index array")
        t, tp = _idx(target)
        self._check(self.lib.vmd_ir_add_sdf(self.h, name.encode(), s.ctypes.data_as(L.c_int32_p), s.shape[0], s.shape[1],
                                            tp, t.size, float(cutoff)))

    def add_sdf_shell(self, name, structures, target, cutoff, target_shell=None):
        """`name = sdf(structures, target and within(a:b, R), cutoff)`: the target may be a shell, given as (R, r_min, r_max) -
        per frame, only the atoms of `target` with some atom of R at r_min <= d < r_max are scattered.  None: add_sdf."""
        import ctypes as C
        s = np.ascontiguousarray(structures, dtype=np.int32)
        if s.ndim != 2:
            raise ValueError("structures must be a [K, m] index array")
        t, tp = _idx(target)
        ptr = None
        if target_shell is not None:
            x, xp = _idx(target_shell[0])
            c = L.ShellC(xp, x.size, float(target_shell[1]), float(target_shell[2]))
            ptr = C.byref(c)
        self._check(self.lib.vmd_ir_add_sdf_shell(self.h, name.encode(), s.ctypes.data_as(L.c_int32_p), s.shape[0], s.shape[1],
                                                  tp, t.size, ptr, float(cutoff)))

    def _shell_expr(self, terms, truth):
        """[(R, r_min, r_max), ...] and a truth table -> a vmd_shell_expr_t and what keeps its lists alive"""
        import ctypes as C
        keep = [_idx(t[0]) for t in terms]
        arr = (L.ShellC * max(len(terms), 1))(*[L.ShellC(k[1], k[0].size, float(t[1]), float(t[2])) for k, t in zip(keep, terms)])
        return L.ShellExprC(C.cast(arr, C.POINTER(L.ShellC)), len(terms), int(truth)), (keep, arr)

    def add_within_count_expr(self, name, target, terms, truth):
        """`name = count(target and <and / or / not over within() terms>);`: terms = up to four (R, r_min, r_max); per frame,
        h_i says whether an atom of `target` is in term i, and it is counted iff bit sum(h_i << i) of `truth` is set.  One term with
        truth 0b10 is add_within_count."""
        import ctypes as C
        t, tp = _idx(target)
        x, keep = self._shell_expr(terms, truth)
        self._check(self.lib.vmd_ir_add_within_count_expr(self.h, name.encode(), tp, t.size, C.byref(x)))

    def add_sdf_shell_expr(self, name, structures, target, cutoff, terms, truth):
        """`name = sdf(structures, target and <and / or / not over within() terms>, cutoff);`: only the members of the
        expression (add_within_count_expr) are scattered.  One term with truth 0b10 is add_sdf_shell."""
        import ctypes as C
        s = np.ascontiguousarray(structures, dtype=np.int32)
        if s.ndim != 2:
            raise ValueError("structures must be a [K, m] index array")
        t, tp = _idx(target)
        x, keep = self._shell_expr(terms, truth)
        self._check(self.lib.vmd_ir_add_sdf_shell_expr(self.h, name.encode(), s.ctypes.data_as(L.c_int32_p), s.shape[0], s.shape[1],
                                                       tp, t.size, C.byref(x), float(cutoff)))

    def add_distance(self, name, a, b, kind=L.DIST_COM):
        """`name = distance|distance_min|distance_max|distance_pair(a, b)` (src/main.cpp:2817-2858)."""
        a_, ap = _idx(a)
        b_, bp = _idx(b)
        self._check(self.lib.vmd_ir_add_distance(self.h, name.encode(), int(kind), ap, a_.size, bp, b_.size))

    def add_distance_population(self, name, a_sets, b_sets, kind=L.DIST_COM):
        """`name = distance*(a, b) in <contexts>`: one (a, b) pair of index sets per context -> dim[1] = number of contexts."""
        assert len(a_sets) == len(b_sets) and len(a_sets) > 0
        a = np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in a_sets]).astype(np.int32)
        b = np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in b_sets]).astype(np.int32)
        ao = np.concatenate([[0], np.cumsum([len(x) for x in a_sets])]).astype(np.int32)
        bo = np.concatenate([[0], np.cumsum([len(x) for x in b_sets])]).astype(np.int32)
        self._check(self.lib.vmd_ir_add_distance_population(self.h, name.encode(), int(kind), len(a_sets),
                                                            a.ctypes.data_as(L.c_int32_p), ao.ctypes.data_as(L.c_int32_p),
                                                            b.ctypes.data_as(L.c_int32_p), bo.ctypes.data_as(L.c_int32_p)))

    def add_angle(self, name, a, b, c):
        """`name = angle(a, b, c);` (DESIGN S6b): the angle at the centre of b, degrees unless spec_angle_radians is set."""
        sets = [_idx(x) for x in (a, b, c)]
        self._check(self.lib.vmd_ir_add_angle(self.h, name.encode(), *[v for x, xp in sets for v in (xp, x.size)]))

    def add_dihedral(self, name, a, b, c, d):
        """`name = dihedral(a, b, c, d);` (DESIGN S6b): IUPAC sign, (-180, 180]."""
        sets = [_idx(x) for x in (a, b, c, d)]
        self._check(self.lib.vmd_ir_add_dihedral(self.h, name.encode(), *[v for x, xp in sets for v in (xp, x.size)]))

    def _add_geometry_population(self, fn, name, arg_sets):
        P = len(arg_sets[0])
        assert P > 0 and all(len(s) == P for s in arg_sets)
        args, keep = [], []
        for sets in arg_sets:
            flat = np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in sets]).astype(np.int32)
            off = np.concatenate([[0], np.cumsum([len(x) for x in sets])]).astype(np.int32)
            keep += [flat, off]
            args += [flat.ctypes.data_as(L.c_int32_p), off.ctypes.data_as(L.c_int32_p)]
        self._check(fn(self.h, name.encode(), P, *args))

    def add_angle_population(self, name, a_sets, b_sets, c_sets):
        """`name = angle(a, b, c) in <contexts>`: one (a, b, c) triple of index sets per context -> dim[1] = number of contexts."""
        self._add_geometry_population(self.lib.vmd_ir_add_angle_population, name, (a_sets, b_sets, c_sets))

    def add_dihedral_population(self, name, a_sets, b_sets, c_sets, d_sets):
        """`name = dihedral(a, b, c, d) in <contexts>`: one quadruple of index sets per context."""
        self._add_geometry_population(self.lib.vmd_ir_add_dihedral_population, name, (a_sets, b_sets, c_sets, d_sets))

    def add_shape_weights(self, names, idx):
        """`{n0, n1, n2} = shape_weights(idx);`: three temporal properties - linear, planar, isotropic - of one set."""
        x, xp = _idx(idx)
        self._check(self.lib.vmd_ir_add_shape_weights(self.h, self._names3(names), xp, x.size))

    def add_shape_weights_population(self, names, sets):
        """`{n0, n1, n2} = shape_weights(sel) in <contexts>`: one index set per context -> dim[1] = number of contexts."""
        assert len(sets) > 0
        flat = np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in sets]).astype(np.int32)
        off = np.concatenate([[0], np.cumsum([len(x) for x in sets])]).astype(np.int32)
        self._check(self.lib.vmd_ir_add_shape_weights_population(self.h, self._names3(names), len(sets), flat.ctypes.data_as(L.c_int32_p),
                                                                 off.ctypes.data_as(L.c_int32_p)))

    def add_rmsd(self, name, idx):
        """`name = rmsd(idx);`: the RMSD of one set from its pose at trajectory frame 0 after the best rigid fit."""
        x, xp = _idx(idx)
        self._check(self.lib.vmd_ir_add_rmsd(self.h, name.encode(), xp, x.size))

    def add_rmsd_population(self, name, sets):
        """`name = rmsd(sel) in <contexts>`: one index set per context -> dim[1] = number of contexts."""
        assert len(sets) > 0
        flat = np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in sets]).astype(np.int32)
        off = np.concatenate([[0], np.cumsum([len(x) for x in sets])]).astype(np.int32)
        self._check(self.lib.vmd_ir_add_rmsd_population(self.h, name.encode(), len(sets), flat.ctypes.data_as(L.c_int32_p),
                                                        off.ctypes.data_as(L.c_int32_p)))

    def add_rmsf(self, name, idx, offsets=None):
        """rmsf: the per-atom residual of rmsd's fit accumulated over the evaluated frames, one record of u64 accumulators
        [ntot + 1, 4].  idx: the set; offsets: P + 1 context offsets into idx for a population (None: one set)."""
        x, xp = _idx(idx)
        if offsets is None:
            self._check(self.lib.vmd_ir_add_rmsf(self.h, name.encode(), xp, x.size))
            return
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        self._check(self.lib.vmd_ir_add_rmsf_population(self.h, name.encode(), max(off.size, 1) - 1, xp,
                                                        off.ctypes.data_as(L.c_int32_p) if off.size else None))

    def add_hbonds(self, names, donors, hydrogens, acceptors, r_da, angle_min_deg):
        """Hydrogen bonds: names = (count per frame, occupancy record); pair j is the heavy atom donors[j] with its explicit
        hydrogen hydrogens[j]; a bond is a (pair, acceptor) combination with d(D, A) within r_da and the D-H...A angle at least
        angle_min_deg.  The record is u64 [npairs + nacc + 1]: per pair, per acceptor, the frames."""
        names = list(names)
        assert len(names) == 2, "hbonds defines two properties"
        d_, dp = _idx(donors)
        h_, hp = _idx(hydrogens)
        a_, ap = _idx(acceptors)
        if d_.size != h_.size:
            raise ValueError("donors and hydrogens must list one atom per pair each")
        sites = L.HbondSitesC(d_.size, dp, hp, a_.size, ap)
        self._check(self.lib.vmd_ir_add_hbonds(self.h, (C.c_char_p * 2)(*[x.encode() for x in names]), C.byref(sites), float(r_da),
                                               float(angle_min_deg)))
        self.hbond_pairs_of = dict(getattr(self, "hbond_pairs_of", {}), **{names[1]: int(d_.size)})

    def add_sasa(self, names, atoms, radii, measured=None, probe=1.4, npoints=96):
        """Solvent-accessible surface area by Shrake-Rupley: names = (area per frame in A^2, record of accessible points).
        atoms / radii: the environment, every atom that occludes, with its van der Waals radius.  measured: positions INTO `atoms` of the
        entries whose area is reported (None: all of them) - the measured set is a subset of the environment.  The record is u64
        [nmeas + 1]: per measured entry the accessible points summed over the evaluated frames, then the frames."""
        a_, _ = _idx(atoms)
        r_ = np.ascontiguousarray(radii, np.float32).reshape(-1)
        if a_.size != r_.size:
            raise ValueError("atoms and radii must list one value per entry each")
        sel = np.arange(a_.size) if measured is None else np.asarray(measured, np.int64).reshape(-1)
        self.add_sasa_lists(names, a_[sel], r_[sel], a_, r_, probe, npoints)

    def add_sasa_lists(self, names, measured, measured_radius, env, env_radius, probe=1.4, npoints=96):
        """vmd_ir_add_sasa as it is: two independent lists of (atom, radius) - the entries whose area is reported, the entries that
        occlude.  An atom in both lists is itself, by index."""
        names = list(names)
        assert len(names) == 2, "sasa defines two properties"
        m_, mp = _idx(measured)
        e_, ep = _idx(env)
        mr = np.ascontiguousarray(measured_radius, np.float32).reshape(-1)
        er = np.ascontiguousarray(env_radius, np.float32).reshape(-1)
        if m_.size != mr.size or e_.size != er.size:
            raise ValueError("every list entry needs one radius")
        sites = L.SasaSitesC(m_.size, mp, mr.ctypes.data_as(L.c_float_p) if mr.size else None,
                             e_.size, ep, er.ctypes.data_as(L.c_float_p) if er.size else None)
        self._check(self.lib.vmd_ir_add_sasa(self.h, (C.c_char_p * 2)(*[x.encode() for x in names]), C.byref(sites), float(probe),
                                             int(npoints)))

    def add_contacts(self, names, atoms, groups, r_cut=4.5, min_sep=3, native=None, ngroups=None):
        """Residue contact maps and the native-contact fraction: names = (pairs in contact per frame, record of the map[,
        Q per frame]).  Entry i is atoms[i] standing for group groups[i]; groups g < h are in contact in a frame when h - g >= min_sep and
        some entry of each is within r_cut of the other.  native: [n, 2] group pairs of the reference set (None / empty: no third name).
        ngroups: None = max(groups) + 1.  The record is u64 [P + 1], P = G (G - 1) / 2 in SciPy's pdist order, then the frames."""
        names = list(names)
        a_, ap = _idx(atoms)
        g_, gp = _idx(groups)
        if a_.size != g_.size:
            raise ValueError("atoms and groups must list one value per entry each")
        nat = np.zeros((0, 2), np.int32) if native is None else np.ascontiguousarray(native, np.int32).reshape(-1, 2)
        assert len(names) == (3 if nat.shape[0] else 2), "contacts defines two properties, three with a native list"
        G = int(ngroups) if ngroups is not None else (int(g_.max()) + 1 if g_.size else 0)
        sites = L.ContactSitesC(a_.size, ap, gp, G, nat.shape[0], nat.ctypes.data_as(L.c_int32_p) if nat.shape[0] else None)
        cn = (C.c_char_p * 3)(*([x.encode() for x in names] + [None] * (3 - len(names))))
        self._check(self.lib.vmd_ir_add_contacts(self.h, cn, C.byref(sites), float(r_cut), int(min_sep)))

    def add_clusters(self, names, atoms, groups, r_cut=3.5, ngroups=None):
        """Connected clusters of groups per frame: names = (clusters per frame, record of the cluster sizes, largest cluster
        per frame).  Entry i is atoms[i] standing for group groups[i]; groups are bonded in a frame when some entry of each is within r_cut
        of the other, and the clusters are the connected components over all groups.  ngroups: None = max(groups) + 1; every group needs an
        entry.  The record is u64 [G + 1]: row s - 1 the clusters of s groups summed over the evaluated frames, then the frames."""
        names = list(names)
        assert len(names) == 3, "clusters defines three properties"
        a_, ap = _idx(atoms)
        g_, gp = _idx(groups)
        if a_.size != g_.size:
            raise ValueError("atoms and groups must list one value per entry each")
        G = int(ngroups) if ngroups is not None else (int(g_.max()) + 1 if g_.size else 0)
        sites = L.ContactSitesC(a_.size, ap, gp, G, 0, None)
        self._check(self.lib.vmd_ir_add_clusters(self.h, (C.c_char_p * 3)(*[x.encode() for x in names]), C.byref(sites), float(r_cut)))

    def add_msd(self, name, atoms):
        """The position table of `atoms`: one TEMPORAL property of 3 n + 9 floats per frame - x, y, z of the atoms as the
        frame holds them, then the frame's cell -, kept on the device for the whole trajectory; ScriptEval.msd correlates it."""
        a_, ap = _idx(atoms)
        self._check(self.lib.vmd_ir_add_msd(self.h, name.encode(), ap, a_.size))

    def add_within_count(self, name, target, ref, rmin, rmax):
        """`name = count(target and within(rmin:rmax, ref));`: per frame, how many atoms of `target` have some atom of `ref`
        (itself included) at rmin <= d < rmax."""
        t, tp = _idx(target)
        r, rp = _idx(ref)
        self._check(self.lib.vmd_ir_add_within_count(self.h, name.encode(), tp, t.size, rp, r.size, float(rmin), float(rmax)))

    def add_ramachandran(self, names, n, ca, c, range_offsets, rama_class=None):
        """`{table, map} = ramachandran(backbone)`: names = (angle table, density map); n / ca / c: the backbone atoms per
        segment; range_offsets: num_ranges + 1 segment offsets of the chains; rama_class: one byte per segment, 0..3 = general, glycine,
        proline, pre-proline, 255 = never binned (None: all general)."""
        names = list(names)
        assert len(names) == 2, "ramachandran defines two properties"
        n_, np_ = _idx(n)
        a_, ap = _idx(ca)
        c_, cp = _idx(c)
        if not (n_.size == a_.size == c_.size):
            raise ValueError("n, ca and c must list one atom per segment each")
        off = np.ascontiguousarray(range_offsets, dtype=np.uint32).reshape(-1)
        cls = None if rama_class is None else np.ascontiguousarray(rama_class, dtype=np.uint8).reshape(-1)
        if cls is not None and cls.size != n_.size:
            raise ValueError("rama_class must hold one byte per segment")
        bb = L.BackboneC(n_.size, np_, ap, cp, max(off.size, 1) - 1, off.ctypes.data_as(C.POINTER(C.c_uint32)) if off.size else None,
                         cls.ctypes.data_as(L.c_uint8_p) if cls is not None else None)
        self._check(self.lib.vmd_ir_add_ramachandran(self.h, (C.c_char_p * 2)(*[x.encode() for x in names]), C.byref(bb)))

    def add_secondary_structure(self, names, n, ca, c, o, offsets, cls=None):
        """`{classes, populations} = secondary_structure(backbone, o)`: names = (class table, populations); n / ca / c / o:
        the backbone atoms per segment, o = -1 where a segment has no carbonyl oxygen; offsets: num_ranges + 1 segment offsets of the
        chains; cls: the rama_class bytes of add_ramachandran, of which 2 marks a proline (None: no proline)."""
        names = list(names)
        assert len(names) == 2, "secondary_structure defines two properties"
        n_, np_ = _idx(n)
        a_, ap = _idx(ca)
        c_, cp = _idx(c)
        o_, op = (None, None) if o is None else _idx(o)
        if not (n_.size == a_.size == c_.size) or (o_ is not None and o_.size != n_.size):
            raise ValueError("n, ca, c and o must list one atom per segment each")
        off = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
        cl = None if cls is None else np.ascontiguousarray(cls, dtype=np.uint8).reshape(-1)
        if cl is not None and cl.size != n_.size:
            raise ValueError("cls must hold one byte per segment")
        bb = L.BackboneC(n_.size, np_, ap, cp, max(off.size, 1) - 1, off.ctypes.data_as(C.POINTER(C.c_uint32)) if off.size else None,
                         cl.ctypes.data_as(L.c_uint8_p) if cl is not None else None)
        self._check(self.lib.vmd_ir_add_secondary_structure(self.h, (C.c_char_p * 2)(*[x.encode() for x in names]), C.byref(bb), op))

    @staticmethod
    def _names3(names):
        import ctypes as C
        names = list(names)
        assert len(names) == 3, "shape_weights defines three properties"
        return (C.c_char_p * 3)(*[n.encode() for n in names])

    def geometry_atoms(self, name, context=-1):
        """the atoms of an angle / dihedral property (one context, or all when context < 0) in argument order, or the set of a
        shape_weights or rmsd property, or the reference set followed by the target set of a within count"""
        n = int(self.lib.vmd_ir_geometry_atoms(self.h, name.encode(), int(context), None, 0))
        out = np.zeros(n, np.int32)
        if n:
            self.lib.vmd_ir_geometry_atoms(self.h, name.encode(), int(context), out.ctypes.data_as(L.c_int32_p), n)
        return out

    def valid(self):
        return bool(self.lib.vmd_ir_valid(self.h))

    def fingerprint(self):
        return int(self.lib.vmd_ir_fingerprint(self.h))

    def property_count(self):
        return int(self.lib.vmd_ir_property_count(self.h))

    def property_names(self):
        n = self.property_count()
        p = self.lib.vmd_ir_property_names(self.h)
        return [p[i].decode() for i in range(n)]

    def property_flags(self, name):
        return int(self.lib.vmd_ir_property_flags(self.h, name.encode()))


class _EvalArray(np.ndarray):
    """ndarray view into memory owned by a ScriptEval: keeps the eval alive for as long as the view (or a slice of it) is."""

    def __array_finalize__(self, obj):
        self._owner = getattr(obj, "_owner", None)


class PropertyDataView:
    """Zero-copy numpy views of one md_script_property_data_t.  The arrays stay valid for the lifetime of the
    eval (md_script_property_data_t addresses are stable, src/main.cpp:1286,1303) and hold a reference to it."""

    def __init__(self, c, ev=None, name=None):
        self.c = c  # ctypes PropertyData (owned by the eval)
        self._ev, self._name = ev, name

    @property
    def dim(self):
        return tuple(self.c.dim)

    @property
    def fingerprint(self):
        return int(self.c.fingerprint)

    def _arr(self, ptr, n, dtype):
        if not ptr or n == 0:
            return None
        a = np.ctypeslib.as_array(ptr, shape=(n,)).view(dtype).view(_EvalArray)
        a._owner = self._ev
        return a

    @property
    def values(self):
        return self._arr(self.c.values, self.c.num_values, np.float32)

    @property
    def weights(self):
        return self._arr(self.c.weights, self.c.dim[2], np.float32) if self.c.weights else None

    @property
    def counts(self):
        if not self.c.counts:
            return None
        if self._ev is not None and not self._ev.lib.vmd_eval_refresh_counts(self._ev.h, self._name.encode()):
            raise VmdError(self._ev.lib.last_error())
        n = self.c.dim[2] if self.c.weights else self.c.dim[1] * self.c.dim[2] * self.c.dim[3]
        return self._arr(self.c.counts, n, np.uint64)

    @property
    def is_map(self):
        """a Ramachandran class map (VMD_PROPERTY_FLAG_MAP): dim = (1, 4, 512, 512), channel fastest"""
        return tuple(self.c.dim) == (1, L.RAMA_MAP_CLASSES, L.RAMA_MAP_DIM, L.RAMA_MAP_DIM)

    @property
    def map_values(self):
        """a MAP property's float view as [y, x, class]"""
        assert self.is_map
        return self.values.reshape(L.RAMA_MAP_DIM, L.RAMA_MAP_DIM, L.RAMA_MAP_CLASSES)

    @property
    def map_counts(self):
        """a MAP property's u64 accumulators as [y, x, class]"""
        assert self.is_map
        return self.counts.reshape(L.RAMA_MAP_DIM, L.RAMA_MAP_DIM, L.RAMA_MAP_CLASSES)

    def _record(self, n):
        """the n uint64 words of a record, brought up to date from the device first"""
        if self._ev is not None and not self._ev.lib.vmd_eval_refresh_counts(self._ev.h, self._name.encode()):
            raise VmdError(self._ev.lib.last_error())
        return self._arr(self.c.counts, n, np.uint64)

    @property
    def rmsf_accumulators(self):
        """the record of an rmsf property as uint64 [ntot + 1, 4]: per entry of the set the two's-complement sums of
        q(d_x), q(d_y), q(d_z) and the sum of q2(|d|^2); the last row's first word is the number of frames accumulated"""
        assert self.c.dim[1] == 4 and self.c.dim[2] == 0, "not an rmsf record"
        return self._record(self.c.dim[0] * 4).reshape(self.c.dim[0], 4)

    @property
    def hbond_accumulators(self):
        """the record of a hydrogen-bond occupancy as uint64 [npairs + nacc + 1]: the bonds every pair donated, the bonds
        every acceptor accepted, the frames accumulated"""
        assert self.c.dim[1] == 1 and self.c.dim[2] == 0 and self.c.counts, "not a hydrogen-bond occupancy record"
        return self._record(self.c.dim[0])

    @property
    def sasa_accumulators(self):
        """the record of a sasa statement as uint64 [nmeas + 1]: the accessible points of every measured entry summed over
        the evaluated frames, the frames accumulated"""
        assert self.c.dim[1] == 1 and self.c.dim[2] == 0 and self.c.counts, "not a record of accessible surface points"
        return self._record(self.c.dim[0])

    @property
    def contact_accumulators(self):
        """the record of a contact map as uint64 [P + 1]: per group pair, in condensed order, the evaluated frames in which
        it was in contact, then the frames accumulated"""
        assert self.c.dim[1] == 1 and self.c.dim[2] == 0 and self.c.counts, "not the record of a contact map"
        return self._record(self.c.dim[0])

    @property
    def cluster_accumulators(self):
        """the record of a cluster statement as uint64 [G + 1]: row s - 1 the clusters of s groups summed over the evaluated
        frames, then the frames accumulated"""
        assert self.c.dim[1] == 1 and self.c.dim[2] == 0 and self.c.counts, "not the record of cluster sizes"
        if self._ev is not None and not self._ev.lib.vmd_eval_refresh_counts(self._ev.h, self._name.encode()):
            raise VmdError(self._ev.lib.last_error())
        return self._arr(self.c.counts, self.c.dim[0], np.uint64)

    @property
    def msd_table(self):
        """the position table of an msd statement as float32 [frames, 3 n + 9]: x[n], y[n], z[n], then the cell's nine"""
        return self.values.reshape(self.c.dim[0], self.c.dim[1])

    @property
    def ss_classes(self):
        """the class table of a secondary_structure statement as uint8 [frames, nseg]: the VMD_SS_* codes, 0 = a frame that
        was not evaluated (a copy: the float rows hold the codes exactly)"""
        return self.values.reshape(self.c.dim[0], self.c.dim[1]).astype(np.uint8)

    @property
    def weights64(self):
        return self._arr(self.c.weights64, self.c.dim[2], np.float64) if self.c.weights64 else None

    @property
    def unit_str(self):
        """(x unit, y unit) as VIAMD prints md_script_property_data_t::unit (src/main.cpp:1314-1315)"""
        return tuple((u or b"").decode("utf-8") for u in self.c.unit_str)

    @property
    def min_range(self):
        return tuple(self.c.min_range)

    @property
    def max_range(self):
        return tuple(self.c.max_range)

    @property
    def max_value(self):
        return float(self.c.max_value)

    @property
    def min_value(self):
        return float(self.c.min_value)

    @property
    def aggregate(self):
        if not self.c.aggregate:
            return None
        a = self.c.aggregate.contents
        n = a.num_values
        def own(arr):
            arr = arr.view(_EvalArray)
            arr._owner = self._ev
            return arr
        return {"mean": own(np.ctypeslib.as_array(a.population_mean, shape=(n,))),
                "var": own(np.ctypeslib.as_array(a.population_var, shape=(n,))),
                "ext": own(np.ctypeslib.as_array(a.population_ext, shape=(n * 2,))).reshape(n, 2)}


class MsdResult(tuple):
    """(msd, per_axis, terms) of ScriptEval.msd, with the raw sums (.sums) and the window's frames (.frames_used)"""
    sums = None
    frames_used = 0


def diffusion_coefficient(msd, dt_ps, lo=0.2, hi=0.8, dims=3):
    """The diffusion coefficient read off an MSD curve: the least-squares slope of msd over the lags tau with
    lo * T <= tau <= hi * T, T = len(msd) - 1 the largest lag, divided by 2 dims (Einstein) -> in msd's unit per ps (A^2 / ps; x 1e-4
    for cm^2 / s).  dt_ps: the time between two frames.  Plain NumPy; needs at least two lags in the range."""
    y = np.asarray(msd, np.float64).reshape(-1)
    T = y.size - 1
    k = np.arange(y.size)
    sel = (k >= lo * T) & (k <= hi * T)
    if sel.sum() < 2:
        raise ValueError("diffusion_coefficient: fewer than two lags in the fit range")
    t = k[sel] * float(dt_ps)
    tc, yc = t - t.mean(), y[sel] - y[sel].mean()
    return float((tc * yc).sum() / (tc * tc).sum()) / (2.0 * dims)


class ScriptEval:
    """md_script_eval_t stand-in: owns the accumulators, evaluates frame ranges on the GPU."""

    def __init__(self, num_frames, ir):
        self.lib = ir.lib
        self.ir = ir
        self.h = self.lib.vmd_eval_create(int(num_frames), ir.h)
        if not self.h:
            raise VmdError(self.lib.last_error())

    def close(self):
        if self.h:
            self.lib.vmd_eval_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear_data(self):
        self.lib.vmd_eval_clear_data(self.h)

    def interrupt(self):
        self.lib.vmd_eval_interrupt(self.h)

    def ir_fingerprint(self):
        return int(self.lib.vmd_eval_ir_fingerprint(self.h))

    def frame_range(self, sys, traj, frame_beg, frame_end):
        """md_script_eval_frame_range(eval, ir, &sys, traj, beg, end); False on interrupt; raises on error."""
        sysp = C.byref(sys.c) if sys is not None else None
        # deferred-settle mode: the helper thread evaluates from copies of these records after the call has returned: the
        # objects behind them - coordinate arrays, ctypes callbacks - stay referenced until the next call, wait_settled, clear_data or free
        self._last_inputs = (sys, traj)
        ok = self.lib.vmd_eval_frame_range(self.h, self.ir.h, sysp, traj.interface(), int(frame_beg), int(frame_end))
        if not ok:
            if self.lib.vmd_eval_frames_done(self.h) < self.num_frames() and self._interrupted():
                return False
            raise VmdError(self.lib.last_error())
        return True

    def _interrupted(self):
        # an interrupt leaves no error message behind
        return True if not self.lib.last_error() else False

    def property_data(self, name):
        p = self.lib.vmd_eval_property_data(self.h, name.encode())
        if not p:
            return None
        return PropertyDataView(p.contents, self, name)

    def set_block_frames(self, block_frames):
        """Keep one partial accumulator per block of `block_frames` frames in HBM (filtered evaluation)."""
        if not self.lib.vmd_eval_set_block_frames(self.h, int(block_frames)):
            raise VmdError(self.lib.last_error())

    def set_source(self, source):
        """Serve whole frame blocks of later frame_range calls from `source`'s block partials (None detaches).
        The VIAMD "Eval Filt" pattern: a second eval over a timeline sub-range (src/main.cpp:1014-1039)."""
        if not self.lib.vmd_eval_set_source(self.h, source.h if source is not None else None):
            raise VmdError(self.lib.last_error())
        self._source = source          # keep it alive

    def frame_stats(self):
        """(frames evaluated by kernels, frames served from block partials) since the last clear_data."""
        a, b = C.c_size_t(0), C.c_size_t(0)
        self.lib.vmd_eval_frame_stats(self.h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def readahead_stats(self):
        """What read-ahead did for this eval (vmd_eval_readahead_stats): a dict of the counters."""
        st = L.ReadAheadStats()
        self.lib.vmd_eval_readahead_stats(self.h, C.byref(st))
        return {k: int(getattr(st, k)) for k, _ in L.ReadAheadStats._fields_}

    def cell_build_stats(self):
        """(bucket overflows of the two-level cell build, selections that left it for the single-level builds)"""
        a, b = C.c_size_t(0), C.c_size_t(0)
        self.lib.vmd_eval_cell_build_stats(self.h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def frames_device_decoded(self):
        """Frames whose coordinates were decompressed on the device (load_raw + k_xtc_decode) since the last clear_data."""
        return int(self.lib.vmd_eval_frames_device_decoded(self.h))

    def frames_section_decoded(self):
        """... and how many of those were decoded in sections from the trajectory's decoder checkpoints (a re-evaluation)."""
        return int(self.lib.vmd_eval_frames_section_decoded(self.h))

    def frames_mapped(self):
        """... and how many reached the device by DMA straight out of the mapped file (no host copy of the compressed bytes)."""
        return int(self.lib.vmd_eval_frames_mapped(self.h))

    def num_frames(self):
        return int(self.lib.vmd_eval_num_frames(self.h))

    def frames_done(self):
        return int(self.lib.vmd_eval_frames_done(self.h))

    def frame_mask(self):
        n = self.num_frames()
        m = np.ctypeslib.as_array(self.lib.vmd_eval_frame_mask(self.h), shape=(n,)).view(_EvalArray)
        m._owner = self
        return m

    def frame_mask_bits(self):
        """the mask as md_bitfield_t storage: uint64 words, bit f & 63 of word f // 64"""
        nw = int(self.lib.vmd_eval_frame_mask_bits(self.h, None, 0))
        w = np.zeros(nw, np.uint64)
        self.lib.vmd_eval_frame_mask_bits(self.h, w.ctypes.data_as(L.c_uint64_p), nw)
        return w

    def set_frame_mask(self, mask):
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        self.lib.vmd_eval_set_frame_mask(self.h, m.ctypes.data_as(L.c_uint8_p), m.size)

    def frame_range_pooled(self, sys, traj, frame_beg, frame_end, num_threads=16, grain=1):
        """VIAMD's call pattern (src/main.cpp:993-997): native pool threads pulling ranges of `grain` frames, all calling frame_range on this eval"""
        sysp = C.byref(sys.c) if sys is not None else None
        self._last_inputs = (sys, traj)
        ok = self.lib.vmd_eval_frame_range_pooled(self.h, self.ir.h, sysp, traj.interface(), int(frame_beg), int(frame_end), int(num_threads), int(grain))
        if not ok:
            if self.lib.vmd_eval_frames_done(self.h) < self.num_frames() and self._interrupted():
                return False
            raise VmdError(self.lib.last_error())
        return True

    def set_deferred_settle(self, mode=1):
        """this eval's own choice of the deferred-settle mode: 1 on, 0 off, -1 follow the process-wide option readahead_lone"""
        if not self.lib.vmd_eval_set_deferred_settle(self.h, int(mode)):
            raise VmdError(self.lib.last_error())

    def wait_settled(self):
        """deferred-settle mode (option readahead_lone): bring totals and views up to what the calls so far asked for, now"""
        if not self.lib.vmd_eval_wait_settled(self.h):
            raise VmdError(self.lib.last_error())

    def defer_volume_views(self, defer=True):
        """a rank of a multi-GPU evaluation: the float view of a volume is derived once, by finalize() / the merge, not after every range"""
        if not self.lib.vmd_eval_defer_volume_views(self.h, bool(defer)):
            raise VmdError(self.lib.last_error())

    def finalize(self):
        if not self.lib.vmd_eval_finalize(self.h):
            raise VmdError(self.lib.last_error())

    def accum_views(self):
        n = self.lib.vmd_eval_accum_views(self.h, None, 0)
        arr = (L.AccumView * n)()
        self.lib.vmd_eval_accum_views(self.h, arr, n)
        return list(arr)

    def rama_density(self, name, frame_beg, frame_end):
        """VIAMD's filtered Ramachandran map: the density of the evaluated frames of [frame_beg, frame_end), binned on the
        device from the angle table it holds -> (values float32 [512, 512, 4] as [y, x, class], sums uint64 [4])"""
        values = np.zeros((L.RAMA_MAP_DIM, L.RAMA_MAP_DIM, L.RAMA_MAP_CLASSES), np.float32)
        sums = np.zeros(L.RAMA_MAP_CLASSES, np.uint64)
        if not self.lib.vmd_eval_rama_density(self.h, name.encode(), int(frame_beg), int(frame_end), values.ctypes.data_as(L.c_float_p),
                                              sums.ctypes.data_as(L.c_uint64_p)):
            raise VmdError(self.lib.last_error())
        return values, sums

    def msd(self, name, beg=0, end=None, max_lag=None, stride=1):
        """Mean-squared displacement over lag times of the position table `name` over the evaluated frames [beg, end), origins
        every `stride` frames, lags 0 .. max_lag (None: the whole window) -> MsdResult (msd float64 [max_lag + 1], per_axis float64
        [max_lag + 1, 3], terms float64 [max_lag + 1]) in square Angstrom; its .sums holds the raw uint64 [max_lag + 1, 4] (2^-20 A^2 quanta
        along x, y, z and the number of terms), its .frames_used the frames of the window."""
        end = self.num_frames() if end is None else int(end)
        max_lag = max(end - int(beg) - 1, 0) if max_lag is None else int(max_lag)
        for v in (beg, end, max_lag, stride):
            if not 0 <= int(v) <= 0xffffffff:
                raise ValueError("msd arguments must be frame numbers")
        sums = np.zeros((max_lag + 1, 4), np.uint64)
        used = C.c_uint32(0)
        if not self.lib.vmd_eval_msd(self.h, name.encode(), int(beg), end, max_lag, int(stride), sums.ctypes.data_as(L.c_uint64_p),
                                     C.byref(used)):
            raise VmdError(self.lib.last_error())
        terms = sums[:, 3].astype(np.float64)
        per_axis = np.divide(sums[:, :3].astype(np.float64), 1048576.0 * terms[:, None], out=np.zeros((max_lag + 1, 3)), where=terms[:, None] > 0)
        out = MsdResult((per_axis.sum(axis=1), per_axis, terms))
        out.sums, out.frames_used = sums, int(used.value)
        return out

    def rmsf(self, name):
        """an rmsf property read from its record as it stands -> (rmsf float64 [ntot], mean_dev float64 [ntot, 3], frames)"""
        ntot = self.property_data(name).dim[0] - 1
        rmsf, mean = np.zeros(max(ntot, 0), np.float64), np.zeros((max(ntot, 0), 3), np.float64)
        frames = C.c_uint64(0)
        if not self.lib.vmd_eval_rmsf(self.h, name.encode(), rmsf.ctypes.data_as(L.c_double_p), mean.ctypes.data_as(L.c_double_p),
                                      C.byref(frames)):
            raise VmdError(self.lib.last_error())
        return rmsf, mean, int(frames.value)

    def hbonds(self, name, npairs=None):
        """a hydrogen-bond occupancy read from its record as it stands -> (donor_occ float64 [npairs], acc_occ float64
        [nacc], frames).  npairs says where the record's donor rows end (None: what ScriptIR.add_hbonds noted for `name`)"""
        if not self.lib.vmd_eval_hbonds(self.h, name.encode(), None, None, None):      # (the name and the form, before any size is believed)
            raise VmdError(self.lib.last_error())
        n = self.property_data(name).dim[0] - 1
        if npairs is None:
            npairs = getattr(self.ir, "hbond_pairs_of", {}).get(name)
            if npairs is None:
                raise VmdError(f"'{name}' was not defined by add_hbonds of this eval's ir: pass npairs")
        nacc = n - int(npairs)
        if nacc < 0:
            raise ValueError("npairs exceeds the record")
        don, acc = np.zeros(int(npairs), np.float64), np.zeros(nacc, np.float64)
        frames = C.c_uint64(0)
        if not self.lib.vmd_eval_hbonds(self.h, name.encode(), don.ctypes.data_as(L.c_double_p), acc.ctypes.data_as(L.c_double_p),
                                        C.byref(frames)):
            raise VmdError(self.lib.last_error())
        return don, acc, int(frames.value)

    def hbond_pairs(self, name, sys, traj, frame, cap=None):
        """the bonds of one frame, on demand -> int32 [n, 3] of {donor, hydrogen, acceptor} atoms in ascending (pair index,
        acceptor list position) order.  cap: room for that many (None: all of them, asked for twice at the most)"""
        room = 1024 if cap is None else int(cap)
        while True:
            out = np.zeros((max(room, 1), 3), np.int32)
            n = self.lib.vmd_eval_hbond_pairs(self.h, name.encode(), C.byref(sys.c) if sys is not None else None, traj.interface(),
                                              int(frame), out.ctypes.data_as(L.c_int32_p), room)
            if n == C.c_size_t(-1).value:
                raise VmdError(self.lib.last_error())
            if cap is not None or n <= room:
                return out[:min(n, room)].copy()
            room = int(n)

    def sasa(self, name):
        """the mean accessible area per measured entry read from its record as it stands -> (mean_area float64 [nmeas] in
        A^2, frames)"""
        if not self.lib.vmd_eval_sasa(self.h, name.encode(), None, None):      # (the name and the form, before any size is believed)
            raise VmdError(self.lib.last_error())
        area = np.zeros(self.property_data(name).dim[0] - 1, np.float64)
        frames = C.c_uint64(0)
        if not self.lib.vmd_eval_sasa(self.h, name.encode(), area.ctypes.data_as(L.c_double_p), C.byref(frames)):
            raise VmdError(self.lib.last_error())
        return area, int(frames.value)

    def sasa_atoms(self, name, sys, traj, frame):
        """the accessible points of every measured entry in one frame, on demand -> uint32 [nmeas]"""
        failed = C.c_size_t(-1).value
        n = self.lib.vmd_eval_sasa_atoms(self.h, name.encode(), C.byref(sys.c) if sys is not None else None, traj.interface(), int(frame),
                                         None, 0)
        if n == failed:
            raise VmdError(self.lib.last_error())
        out = np.zeros(max(n, 1), np.uint32)
        if self.lib.vmd_eval_sasa_atoms(self.h, name.encode(), C.byref(sys.c) if sys is not None else None, traj.interface(), int(frame),
                                        out.ctypes.data_as(C.POINTER(C.c_uint32)), n) == failed:
            raise VmdError(self.lib.last_error())
        return out[:n].copy()

    def contacts(self, name, square=False):
        """a contact map read from its record as it stands (any name of the statement) -> (occupancy, frames): occupancy
        float64 [P] = count / frames in condensed pair order (SciPy's pdist), or with square=True the symmetric [G, G] matrix with a zero
        diagonal"""
        if not self.lib.vmd_eval_contacts(self.h, name.encode(), None, None):  # (the name and the form, before any size is believed)
            raise VmdError(self.lib.last_error())
        # the statement's record stands behind its count and in front of its native fraction: its rows say P, and P says G.  Of the two
        # temporal names only the count has atoms (vmd_ir_geometry_atoms: the entries' atoms; the native fraction: none) - what stands
        # next to the statement in the ir never enters into it
        names = self.ir.property_names()
        i = names.index(name)
        if self.ir.property_flags(name) != L.FLAG_MAP:
            i = i + 1 if self.ir.geometry_atoms(name).size else i - 1
        P = self.property_data(names[i]).dim[0] - 1
        G = (1 + math.isqrt(1 + 8 * P)) // 2
        assert G * (G - 1) // 2 == P, "not the record of a contact map"
        occ = np.zeros(P, np.float64)
        frames = C.c_uint64(0)
        if not self.lib.vmd_eval_contacts(self.h, name.encode(), occ.ctypes.data_as(L.c_double_p), C.byref(frames)):
            raise VmdError(self.lib.last_error())
        if not square:
            return occ, int(frames.value)
        full = np.zeros((G, G), np.float64)
        iu = np.triu_indices(G, 1)
        full[iu] = occ
        return full + full.T, int(frames.value)

    def contact_pairs(self, name, sys, traj, frame, cap=None):
        """the group pairs in contact in one frame, on demand -> int32 [n, 2] of {g, h}, g < h, in ascending condensed
        index.  cap: room for that many (None: all of them, asked for twice at the most)"""
        room = 1024 if cap is None else int(cap)
        while True:
            out = np.zeros((max(room, 1), 2), np.int32)
            n = self.lib.vmd_eval_contact_pairs(self.h, name.encode(), C.byref(sys.c) if sys is not None else None, traj.interface(),
                                                int(frame), out.ctypes.data_as(L.c_int32_p), room)
            if n == C.c_size_t(-1).value:
                raise VmdError(self.lib.last_error())
            if cap is not None or n <= room:
                return out[:min(n, room)].copy()
            room = int(n)

    def _cluster_groups(self, name):
        """G of the cluster statement that `name` names (any of its three names), from the name's own form: the record is the MAP of the
        three; of the two temporal names only the count has atoms (vmd_ir_geometry_atoms), so the record stands one place behind the count
        and one in front of the largest - what stands next to the statement in the ir never enters into it"""
        if not self.lib.vmd_eval_cluster_sizes(self.h, name.encode(), None, None):     # (the name and the form, before any size is believed)
            raise VmdError(self.lib.last_error())
        names = self.ir.property_names()
        i = names.index(name)
        if self.ir.property_flags(name) != L.FLAG_MAP:
            i = i + 1 if self.ir.geometry_atoms(name).size else i - 1
        return self.property_data(names[i]).dim[0] - 1

    def cluster_sizes(self, name):
        """the cluster sizes read from their record as it stands (any name of the statement) -> (mean_count, frames):
        mean_count float64 [G], entry s - 1 = the clusters of s groups per frame"""
        G = self._cluster_groups(name)
        mean = np.zeros(G, np.float64)
        frames = C.c_uint64(0)
        if not self.lib.vmd_eval_cluster_sizes(self.h, name.encode(), mean.ctypes.data_as(L.c_double_p), C.byref(frames)):
            raise VmdError(self.lib.last_error())
        return mean, int(frames.value)

    def cluster_labels(self, name, sys, traj, frame):
        """the cluster labels of one frame, on demand -> (labels uint32 [G], labels[g] = the lowest group of g's cluster;
        the number of clusters)"""
        G = self._cluster_groups(name)
        labels = np.zeros(G, np.uint32)
        n = self.lib.vmd_eval_cluster_labels(self.h, name.encode(), C.byref(sys.c) if sys is not None else None, traj.interface(),
                                             int(frame), labels.ctypes.data_as(C.POINTER(C.c_uint32)))
        if n == C.c_size_t(-1).value:
            raise VmdError(self.lib.last_error())
        return labels, int(n)

    def sdf_matrices(self, name, sys, traj, frame):
        """vis.sdf.matrices / vis.sdf.extent of md_script_vis_eval_payload (density_volume.cpp:183-204)."""
        K = C.c_size_t(0)
        ext = C.c_float(0)
        sysp = C.byref(sys.c) if sys is not None else None
        if not self.lib.vmd_eval_sdf_matrices(self.h, name.encode(), sysp, traj.interface(), int(frame), None, C.byref(K), C.byref(ext)):
            raise VmdError(self.lib.last_error())
        mats = np.zeros((K.value, 16), np.float32)
        if not self.lib.vmd_eval_sdf_matrices(self.h, name.encode(), sysp, traj.interface(), int(frame),
                                              mats.ctypes.data_as(L.c_float_p), C.byref(K), C.byref(ext)):
            raise VmdError(self.lib.last_error())
        # column-major mat4 -> numpy [K,4,4] with M[k] @ [x,y,z,1]
        return mats.reshape(-1, 4, 4).transpose(0, 2, 1).copy(), float(ext.value)


def _sdf_payload(self, name, sys, traj, frame):
    """md_script_vis_eval_payload(ATOMS | SDF) as VIAMD consumes it: (matrices [K,4,4] with M[k] @ [x,y,z,1], structures [K,m]
    atom indices, extent) - density_volume.cpp:183-204, 263-269."""
    pl = L.SdfPayload()
    sysp = C.byref(sys.c) if sys is not None else None
    if not self.lib.vmd_eval_sdf_payload(self.h, name.encode(), sysp, traj.interface(), int(frame), C.byref(pl)):
        raise VmdError(self.lib.last_error())
    K, m = pl.num_structures, pl.atoms_per_structure
    mats = np.ctypeslib.as_array(pl.matrices, shape=(K, 16)).copy().reshape(K, 4, 4).transpose(0, 2, 1).copy()
    structures = np.ctypeslib.as_array(pl.structures, shape=(K, m)).copy()
    return mats, structures, float(pl.extent)


def _shell_mask(self, name, sys, traj, frame, which=1):
    """the members of a within() shell at one frame (vmd_eval_shell_mask) as bool [num_atoms]; `name` a count(... within ...)
    property, an rdf over shells or an sdf over a shell; which: 0 = the reference argument, 1 = the target argument"""
    n = int(traj.num_atoms())
    words = np.zeros((n + 63) // 64, np.uint64)
    sysp = C.byref(sys.c) if sys is not None else None
    got = self.lib.vmd_eval_shell_mask(self.h, name.encode(), int(which), sysp, traj.interface(), int(frame),
                                       words.ctypes.data_as(C.POINTER(C.c_uint64)), words.size)
    if got == L.SHELL_MASK_FAILED:
        raise VmdError(self.lib.last_error())
    mask = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
    assert int(mask.sum()) == got
    return mask


def _export_cube(self, path, name, sys, traj, frame=0, atomic_numbers=None):
    """export_cube (src/main.cpp:5718-5830) in C++ behind the ABI: the volume + the atoms of reference structure 0."""
    an = None if atomic_numbers is None else np.ascontiguousarray(atomic_numbers, np.uint8)
    sysp = C.byref(sys.c) if sys is not None else None
    if not self.lib.vmd_export_cube(str(path).encode(), self.h, name.encode(), sysp, traj.interface(), int(frame),
                                    an.ctypes.data_as(L.c_uint8_p) if an is not None else None):
        raise VmdError(self.lib.last_error())


def _export_table(self, path, name, fmt="xvg", frame_times=None, num_bins=0, time_unit=None):
    """the XVG / CSV table VIAMD's export window writes for a temporal or distribution property (src/main.cpp:5953-6040)"""
    ft = None if frame_times is None else np.ascontiguousarray(frame_times, np.float64)
    if not self.lib.vmd_export_property_table(str(path).encode(), self.h, name.encode(), fmt.encode(),
                                              ft.ctypes.data_as(L.c_double_p) if ft is not None else None,
                                              time_unit.encode() if time_unit else None, int(num_bins)):
        raise VmdError(self.lib.last_error())


ScriptEval.sdf_payload = _sdf_payload
ScriptEval.shell_mask = _shell_mask
ScriptEval.export_cube = _export_cube
ScriptEval.export_table = _export_table


def downsample_histogram(values, weights, num_bins, lib=None):
    """What VIAMD plots for a distribution property: g = sum(values)/sum(weights) per display bin (src/main.cpp:232-250)."""
    lib = lib or L.default_lib()
    v = np.ascontiguousarray(values, np.float32)
    w = None if weights is None else np.ascontiguousarray(weights, np.float32)
    out = np.zeros(num_bins, np.float32)
    lib.vmd_downsample_histogram(out.ctypes.data_as(L.c_float_p), num_bins, v.ctypes.data_as(L.c_float_p),
                                 w.ctypes.data_as(L.c_float_p) if w is not None else None, v.size)
    return out


def compute_histogram_masked(values, dim, mask, num_bins, rmin, rmax, aggregate=False, lib=None):
    lib = lib or L.default_lib()
    v = np.ascontiguousarray(values, np.float32)
    m = np.ascontiguousarray(mask, np.uint8)
    out = np.zeros((1 if aggregate else dim) * num_bins, np.float32)
    lib.vmd_compute_histogram_masked(out.ctypes.data_as(L.c_float_p), num_bins, float(rmin), float(rmax),
                                     v.ctypes.data_as(L.c_float_p), dim, m.ctypes.data_as(L.c_uint8_p), m.size, bool(aggregate))
    return out


def compute_histogram_masked_y(values, dim, mask, num_bins, rmin, rmax, aggregate=False, lib=None):
    """-> (bins, (y_min, y_max)): compute_histogram_masked plus the value range VIAMD stores with the histogram (src/main.cpp:212-229)."""
    lib = lib or L.default_lib()
    v = np.ascontiguousarray(values, np.float32)
    m = np.ascontiguousarray(mask, np.uint8)
    out = np.zeros((1 if aggregate else dim) * num_bins, np.float32)
    yr = np.zeros(2, np.float32)
    lib.vmd_compute_histogram_masked_y(out.ctypes.data_as(L.c_float_p), num_bins, float(rmin), float(rmax), v.ctypes.data_as(L.c_float_p),
                                       dim, m.ctypes.data_as(L.c_uint8_p), m.size, bool(aggregate), yr.ctypes.data_as(L.c_float_p))
    return out, (float(yr[0]), float(yr[1]))


def compute_histogram(values, num_bins, rmin, rmax, lib=None):
    """-> (bins, min, max): VIAMD's unmasked compute_histogram (src/main.cpp:139-170)."""
    lib = lib or L.default_lib()
    v = np.ascontiguousarray(values, np.float32)
    out = np.zeros(num_bins, np.float32)
    lo, hi = C.c_float(0), C.c_float(0)
    lib.vmd_compute_histogram(out.ctypes.data_as(L.c_float_p), num_bins, float(rmin), float(rmax), v.ctypes.data_as(L.c_float_p), v.size,
                              C.cast(C.byref(lo), L.c_float_p), C.cast(C.byref(hi), L.c_float_p))
    return out, lo.value, hi.value


def scale_histogram(bins, weights, lib=None):
    """bins / weights where the weight is not zero (src/main.cpp:252-261); returns a new array."""
    lib = lib or L.default_lib()
    b = np.array(bins, np.float32)
    w = np.ascontiguousarray(weights, np.float32)
    lib.vmd_scale_histogram(b.ctypes.data_as(L.c_float_p), w.ctypes.data_as(L.c_float_p), b.size)
    return b
