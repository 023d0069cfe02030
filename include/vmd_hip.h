/*
 * include/vmd_hip.h — thin C-ABI layer over the hand-written gfx950 kernels (no host state, no torch types).
 *
 * Every function enqueues work on `stream` (a hipStream_t passed as void*) and returns 0 or a hipError_t.
 * Pointers are device pointers unless a comment says "host".  A *frame batch* is B consecutive frames:
 * frame b has x at xyz + b*frame_stride, y at +row_stride, z at +2*row_stride (floats); boxes[b*9+{0,1,2}]
 * are its cell edge lengths (SPEC S1), boxes[b*9+{3,4,5}] their reciprocals fl(1.0f/L) (SPEC S2) and boxes[b*9+{6,7,8}]
 * the tilt factors xy, xz, yz, all filled by the host.  pbc_flags: bits 0-2 periodic axes, bit 3 triclinic (SPEC S3t;
 * brute / sdf / distance kernels only — the pencil grid is orthorhombic).
 *
 * Reference functions replaced (the sources are in the empty submodule ext/mdlib, /root/reference/.gitmodules:10-12;
 * names from /root/reference/ext/ImGuiColorTextEdit/TextEditor.cpp:3318-3331 and SURVEY.md 8a):
 *   vmd_hip_cells_*   <- md_spatial_hash build            (a5)
 *   vmd_hip_rdf_*     <- rdf() pair loop + md_spatial_hash query (a4, a5)
 *   vmd_hip_sdf_*     <- sdf() alignment + density-volume accumulation (a6, a7, a9)
 *   vmd_hip_distance  <- distance / distance_min / distance_max / distance_pair (a8)
 *   vmd_hip_geometry  <- angle / dihedral (DESIGN S6b)
 *   vmd_hip_shape     <- shape_weights
 *   vmd_hip_rmsd      <- rmsd
 *   vmd_hip_rmsf_*    <- rmsf
 *   vmd_hip_within_*  <- count(sel and within(r, sel))
 *   vmd_hip_within_*_flags, vmd_hip_shell_compact, vmd_hip_rdf_brute_masked  <- rdf() over within() shells
 *   vmd_hip_within_atoms, vmd_hip_within_brute_atoms, vmd_hip_sdf_scatter_masked  <- sdf() over a within() shell, shell masks
 *   vmd_hip_within_atoms_expr, vmd_hip_within_brute_expr, vmd_hip_shell_expr_finish  <- and / or / not over within() shells
 *   vmd_hip_sorted_atoms, vmd_hip_hbond_*  <- hydrogen bonds
 *   vmd_hip_contact_*  <- residue contact maps
 *   vmd_hip_cluster_*  <- connected clusters of groups
 *   vmd_hip_msd_*  <- mean-squared displacement over lag times (the reference has no such code)
 *   vmd_hip_sasa_*  <- solvent-accessible surface area
 *   vmd_hip_xtc_decode <- md_xtc frame decompression (f1; /root/reference/src/loader.cpp:147-148)
 */
#ifndef VMD_HIP_H
#define VMD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* pencil grid of one batch: ny*nz pencils along x, each cut into nxf fine cells (SPEC S3 note) */
typedef struct vmd_grid_t {
    int32_t nxf, ny, nz;
    int32_t ncell;          /* nxf*ny*nz */
} vmd_grid_t;

/* K1: bin the `nsel` selected atoms of every frame of the batch into the grid and write them cell-sorted.
 *   sel        int32[nsel] atom indices (NULL = 0..nsel-1)
 *   cell_count u32[B][ncell+1]  scratch, zeroed by this call
 *   rank       u32[B][nsel]     scratch
 *   cell_start u32[B][ncell+1]  out: exclusive prefix of the cell populations
 *   sorted     f32[B][3][nsel_pad] out: wrapped coordinates in cell order (x row, y row, z row)
 *   aos        f32[B][nsel_pad][4] scratch or NULL: when given, the sort scatters one 16-byte record per atom and a
 *              coalesced repack pass produces `sorted` (fewer scattered L2 transactions) */
/* selections of <= 65536 atoms on grids with ncell + 1 <= 24576 are built by one block per frame entirely in LDS
 * (count -> scan -> scatter); larger ones take the three-kernel path with global atomics */
int vmd_hip_cells_fused_ok(vmd_grid_t grid, int nsel);
int vmd_hip_set_cells_fused(int on);   /* tuning / A-B switch, returns the previous value */
/* selections above 64k atoms: G blocks per frame, each with the cell table in LDS (no global atomics); 0 = not applicable */
int vmd_hip_cells_split_blocks(vmd_grid_t grid, int nsel);
int vmd_hip_set_cells_split(int on);   /* A-B switch, returns the previous value */
/* u32 words per frame the `rank` scratch of vmd_hip_cells_build must hold for this grid and selection */
size_t vmd_hip_cells_scratch_words(vmd_grid_t grid, int nsel);
/* bounding box of all atoms of each frame: out f32[B][6] = {min x,y,z, max x,y,z} (open axes: the grid spans this box) */
int vmd_hip_bbox(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, int B, int natoms, float* out);
/* pbc_flags: bits 0..2 periodic axes, bit 3 triclinic.  On an open axis boxes[b] holds the extent of the batch's bounding box
 * in the L slot, its inverse in the 1/L slot and its origin in slot 6 + axis (the tilt slots, unused without bit 3). */
int vmd_hip_cells_build(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                        const float* boxes, uint32_t pbc_flags, int B, const int32_t* sel, int nsel, int nsel_pad,
                        vmd_grid_t grid, uint32_t* cell_count, uint32_t* rank, uint32_t* cell_start, float* sorted,
                        float* aos);

/* K1, two-level build (the default whenever the grid has <= 4096 pencils): the frame is read once, every atom travels as one
 * 16-byte record {x, y, z, fine cell} through a per-pencil bucket, and one block per (frame, pencil) sorts its bucket in LDS and
 * writes its stretch of `sorted` / `cell_start` coalesced (k_cells_bin, k_cells_pen_scan, k_cells_pen_sort).
 *   pen_off    u32[npen + 1]: exclusive prefix of the bucket capacities in records (npen = ny*nz), chosen by the host from
 *              vmd_hip_cells_pencil_count of a few frames plus head room; every capacity <= vmd_hip_cells_pencil_cap_max()
 *   total_cap  pen_off[npen]; cap_max: the largest capacity
 *   pen_count  u32[B][npen] scratch (zeroed by the call), pen_start u32[B][npen + 1] scratch, bucket f32[B][total_cap][4] scratch
 *   overflow   u32[1]: set to 1 when an atom found its bucket full (never cleared here).  The sorted copy is then incomplete;
 *              vmd_hip_rdf_pencil / vmd_hip_axpy_u64 given the same flag do nothing, the caller enlarges the buckets and repeats */
/* the bit a bucket overflow of the NEXT vmd_hip_cells_build_pencil calls of this host thread ORs into *overflow (default 1): the evaluator
 * gives every selection its own, so that only the selection that overflowed gets wider buckets; returns the previous value */
uint32_t vmd_hip_set_cells_overflow_bit(uint32_t bit);
int vmd_hip_cells_pencil_ok(vmd_grid_t grid);
int vmd_hip_set_cells_pencil(int on);  /* A-B switch (0 = the single-level builds below), returns the previous value */
int vmd_hip_cells_pencil_cap_max(void);
/* atoms per pencil of S frames: counts u32[S][npen], zeroed by the call */
int vmd_hip_cells_pencil_count(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes,
                               uint32_t pbc_flags, int S, const int32_t* sel, int nsel, vmd_grid_t grid, uint32_t* counts);
int vmd_hip_cells_build_pencil(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes,
                               uint32_t pbc_flags, int B, const int32_t* sel, int nsel, int nsel_pad, vmd_grid_t grid,
                               const uint32_t* pen_off, int total_cap, int cap_max, uint32_t* pen_count, uint32_t* pen_start,
                               float* bucket, uint32_t* overflow, uint32_t* cell_start, float* sorted);

/* K2: RDF pair histogram over a batch from cell-sorted selections (ref may equal tgt -> half shell).
 *   partial   u64[vmd_hip_rdf_partial_words()] scratch (per-wave rows + the work counter)
 *   counts    u64[nbins]  accumulated (+=) with device atomics
 *   variant   0 = wave queue (one compaction per candidate column; the default of the evaluator), 1 = inline hit path,
 *             2 = wave queue with pair entries (two columns share one compaction), 3 = 0 behind a bounding-box test of the j
 *             windows; 2 and 3 are measured A/B options (slower), all four give identical counts
 *   pbc_flags as for vmd_hip_cells_build (the same boxes and flags the selections were sorted with).  Triclinic: boxes
 *             carry tilt factors, cells live in the unsheared coordinates s_k * L_k (SPEC S3t) and the grid edge must be
 *             >= rmax measured perpendicular to the cell faces.  Open axes: no images, neighbours end at the bounding box. */
int vmd_hip_rdf_num_blocks(void);
int vmd_hip_set_rdf_pop(int mode);    /* how k_rdf_pencil drains its hit stack when r_min == 0: 0 = the 9-instruction pop, 1 (default) = margin folded into the constant, spare bin, stack read with ds_read_addtid_b32 (6); returns the previous value */
int vmd_hip_set_rdf_shift_axes(int on); /* A-B switch: a periodic-image segment of k_rdf_pencil whose shift has one non-zero axis subtracts that shift alone (default on) instead of all three; same counts; returns the previous value */
int vmd_hip_set_rdf_nsub(int n);       /* tuning knob: work items per pencil (1..64, 0 = automatic), returns the previous value */
int vmd_hip_set_rdf_nsub_pct(int pct);  /* tuning knob: the automatic number of work items per pencil as a percentage of the mean number of i-chunks per pencil */
int vmd_hip_set_rdf_shared_hist(int on); /* A-B switch: one LDS histogram per block instead of one per wave, returns the previous value */
int vmd_hip_set_cells_bin_lds(int on); /* A-B switch: level 1 of the two-level cell build orders a block's records by pencil in LDS and writes
                                        * them as coalesced runs (default on) instead of one scattered record per lane; returns the previous value */
int vmd_hip_set_cells_rec3(int on);   /* A-B switch: 12-byte bucket records {x, y, z} in the two-level cell build where the fine cell follows
                                        * from the wrapped x alone (x-periodic, non-triclinic cells); default on; returns the previous value */
void vmd_hip_set_pencil_reach(int ry, int rz); /* A-B switch: neighbour reach of the pencil walk in y / z (1 = pencils of cross-section >= rmax,
                                                 * 2 = split pencils >= rmax/2: 5 instead of 3 neighbours on that axis, x windows shrunk for the
                                                 * outer ones); process-wide, the grid passed to the cell build and to the walk must be cut to match */
int vmd_hip_set_rdf_blocks(int n);     /* tuning knob: persistent grid size (8..2048), returns the previous value */
size_t vmd_hip_rdf_partial_words(void);
int vmd_hip_rdf_pencil(void* stream, const float* sorted_ref, const uint32_t* cell_start_ref, int nref, int nref_pad,
                       const float* sorted_tgt, const uint32_t* cell_start_tgt, int ntgt, int ntgt_pad,
                       const float* boxes, int B, vmd_grid_t grid, float rmin, float rmax, int nbins,
                       int same_set, int variant, uint32_t pbc_flags, uint64_t* partial, uint64_t* counts,
                       const uint32_t* skip_flag /* device u32 or NULL: non-zero = do nothing (see vmd_hip_cells_build_pencil) */);

/* general RDF (any periodicity flags, any cutoff, no grid): O(nref*ntgt) per frame, SPEC S3 by comparison */
int vmd_hip_rdf_brute(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                      const float* boxes, uint32_t pbc_flags, int B,
                      const int32_t* ref, int nref, const int32_t* tgt, int ntgt,
                      float rmin, float rmax, int nbins, uint64_t* counts);

/* K3: per frame, per reference structure alignment (fp64, SPEC S5).
 *   structs  int32[K][m], mass f32[K][m], ref_pose f64[m][3] (COM-centred)
 *   R32 f32[B][K][9], c32 f32[B][K][3] out;  M64 f64[B][K][12] out (optional, may be NULL)
 *   group f32[B][4] out (optional): centre + radius of the set of structure COMs, the scatter's one-test pre-filter
 *   tree_order, tree_parent  int32[K][m] or both NULL: make every structure whole along its bond tree (atom order[t] hangs on atom
 *          parent[order[t]], local indices, parent < 0 = root) instead of along the index order; tree_pos f64[B*K][m][3] scratch */
int vmd_hip_sdf_align(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                      const float* boxes, uint32_t pbc_flags, int B,
                      const int32_t* structs, const float* mass, int K, int m, const double* ref_pose,
                      float* R32, float* c32, double* M64, float* group,
                      const int32_t* tree_order, const int32_t* tree_parent, double* tree_pos);
/* reference pose from one frame (structure 0): ref_pose f64[m][3] out; tree_order / tree_parent: int32[m] of structure 0 or NULL */
int vmd_hip_sdf_ref_pose(void* stream, const float* xyz, size_t row_stride, const float* box, uint32_t pbc_flags,
                         const int32_t* struct0, const float* mass0, int m, double* ref_pose,
                         const int32_t* tree_order, const int32_t* tree_parent);
/* K4: scatter target atoms of every frame into the dim^3 u64 volume (x fastest), SPEC S5.
 *   owner  int8[ntgt]: index of the structure target t belongs to, -1 if none (NULL: membership is searched in structs;
 *          an atom listed in several structures needs NULL) */
int vmd_hip_sdf_scatter(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                        const float* boxes, uint32_t pbc_flags, int B,
                        const int32_t* structs, int K, int m, const float* R32, const float* c32,
                        const int32_t* tgt, const int8_t* owner, int ntgt, float extent, int dim, uint64_t* volume,
                        const float* group /* from vmd_hip_sdf_align, or NULL */,
                        const uint8_t* atom_tag /* u8[row_stride] or NULL: dense-target path, one tag per ATOM: 255 = not a
                                                   target, 254 = target, k <= 253 = target that belongs to structure k */,
                        int tgt_first, int tgt_stride /* tgt_stride > 0: target t is atom tgt_first + t*tgt_stride (the index list
                                                         is an arithmetic progression: no index load in front of the gathers) */,
                        int unowned /* 1: no target is a member of any structure (owner all -1): skip the owner loads */);
int vmd_hip_set_sdf_rows(int n);       /* tuning knob: row-streaming scatter for progression targets with stride <= 4 (0 = off; 1, 2, 4 groups of 4 atoms per thread) */
int vmd_hip_set_sdf_ilp(int n);        /* tuning knob: target atoms per thread of the scatter (4 or 8), returns the previous value */
int vmd_hip_set_rdf_nsplit(int n);     /* pair launches with fewer work items than resident waves deal a chunk's neighbour pencils to n items each: -1 automatic (5 same-set / 9), 0 off */
int vmd_hip_set_sdf_wave(int on);      /* SDF scatter kernel: 0 = per-block compaction of the group test's survivors, 1 = per wave (no block barrier), 2 = the persistent streaming kernel (a wave walks tiles, next tile's gathers in flight) on 2 048 blocks, n >= 16 = on n blocks */

/* K5: distance family, one row per frame: out f32[B][P*per].  kind as vmd_distance_kind_t; P contexts (population);
 * context c uses a[aoff[c]..aoff[c+1]) and b[boff[c]..boff[c+1]); per = 1 (COM/MIN/MAX) or |a_c|*|b_c| (PAIR, equal
 * for all contexts).  mass_a/mass_b parallel to a/b (COM only). */
int vmd_hip_distance(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                     const float* boxes, uint32_t pbc_flags, int B, int kind, int P, int per,
                     const int32_t* a, const float* mass_a, const int32_t* aoff,
                     const int32_t* b, const float* mass_b, const int32_t* boff, float* out);

/* K5b: angle(a,b,c) (nargs 3) / dihedral(a,b,c,d) (nargs 4), DESIGN S6b: out f32[B][P], one value per frame and context.  Argument k
 * of context c is the S6 centre of sets[k][offsets[k][c] .. offsets[k][c+1]) with masses[k] parallel to sets[k] (device arrays; the
 * three pointer arrays themselves are host arrays of nargs entries).  radians = 0: degrees (D-ANGLE-UNIT). */
int vmd_hip_geometry(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                     const float* boxes, uint32_t pbc_flags, int B, int nargs, int P,
                     const int32_t* const* sets, const float* const* masses, const int32_t* const* offsets, int radians, float* out);

/* K5c: {lin, plan, iso} = shape_weights(sel), DESIGN 1.4: three f32[B][P] blocks, one value per frame and context.  Context c is
 * set[offsets[c] .. offsets[c+1]) with mass parallel to set (device arrays); max_set is the size of the largest context's set.  Sets of
 * more than 64 atoms are summed in chunks through `partial`, a device workspace of vmd_hip_shape_partial_doubles(B, P, max_set)
 * doubles (0 and partial == NULL when max_set <= 64: one wave per set, no workspace). */
size_t vmd_hip_shape_partial_doubles(int B, int P, int max_set);
int vmd_hip_shape(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                  const float* boxes, uint32_t pbc_flags, int B, int P,
                  const int32_t* set, const float* mass, const int32_t* offsets, int max_set,
                  double* partial, float* lin, float* plan, float* iso);

/* K5d: name = rmsd(sel), DESIGN 1.5: one f32[B][P] block, the mass-weighted RMSD of every context's set after the best rigid fit onto
 * its pose at trajectory frame 0.  Context c is set[offsets[c] .. offsets[c+1]) with mass parallel to set (device arrays); max_set is the
 * size of the largest context's set.  vmd_hip_rmsd_pose runs once per trajectory over frame 0 (xyz, box: that one frame) and fills
 * pose (3 doubles per entry of set) and consts (8 doubles per context); vmd_hip_rmsd reads them for every batch.  zero_row is the row
 * of the batch that IS trajectory frame 0 - its values are +0 by definition - or -1.  `workspace` is device memory of
 * vmd_hip_rmsd_workspace_bytes(B, P, max_set) bytes, 8-byte aligned (B = 1 for the pose): the sums of every (frame, context, chunk of
 * 4096 atoms) and the chunks' link shifts; the sums alone when max_set <= 64 (one wave per set). */
size_t vmd_hip_rmsd_workspace_bytes(int B, int P, int max_set);
int vmd_hip_rmsd_pose(void* stream, const float* xyz, size_t row_stride, const float* box, uint32_t pbc_flags, int P,
                      const int32_t* set, const float* mass, const int32_t* offsets, int max_set,
                      void* workspace, double* pose, double* consts);
int vmd_hip_rmsd(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                 const float* boxes, uint32_t pbc_flags, int B, int P,
                 const int32_t* set, const float* mass, const int32_t* offsets, int max_set,
                 const double* pose, const double* consts, int zero_row, void* workspace, float* out);

/* K5e: rmsf, DESIGN 1.13: the per-atom residual of K5d's fit, accumulated over frames in fixed point.  Sets, pose, consts, max_set and
 * workspace as for vmd_hip_rmsd.  vmd_hip_rmsf_fit runs the sums of the batch into `workspace` (have_sums != 0: a vmd_hip_rmsd call over
 * the same sets and batch has left them there) and writes R, ebar and ubar of every (frame, context) to rot, device memory of
 * vmd_hip_rmsf_rot_doubles(B, P) doubles.  vmd_hip_rmsf_accumulate adds frames [b0, b0 + nb) of the batch to acc, u64[offsets[P] + 1][4]:
 * row j = entry j of set, words 0..2 the two's-complement sums of llrint(d 2^24) per axis, word 3 the sum of llrint(min(|d|^2, 2^20) 2^24);
 * the last row's word 0 gains nb.  zero_row: the row of the batch that is trajectory frame 0 (counted, adds nothing), or -1.  groups: the
 * frame groups of the launch, <= 0 for vmd_hip_rmsf_groups' own choice (which is also how a given number is clamped); every choice gives
 * the same record. */
size_t vmd_hip_rmsf_rot_doubles(int B, int P);
int vmd_hip_rmsf_groups(int nb, int P, int max_set, int want);
int vmd_hip_rmsf_fit(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags,
                     int B, int P, const int32_t* set, const float* mass, const int32_t* offsets, int max_set, const double* pose,
                     const double* consts, void* workspace, int have_sums, double* rot);
int vmd_hip_rmsf_accumulate(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes,
                            uint32_t pbc_flags, int B, int P, const int32_t* set, const float* mass, const int32_t* offsets,
                            int max_set, const double* pose, const double* consts, int zero_row, void* workspace,
                            const double* rot, int b0, int nb, int groups, uint64_t* acc);

/* K6: count(T and within(rmin:rmax, R)), DESIGN 1.6: count_out u32[B] (zeroed by the call) = the atoms t of the target set for which SOME
 * atom a of the reference set (a == t included) lies at rmin <= d(t, a) < rmax (closed != 0: <= rmax); positions wrapped (SPEC S2 / S3t),
 * d the correctly rounded root of the SPEC S3 / S3t squared distance - the d the RDF kernels bin.  B <= 65535.
 *   vmd_hip_within_brute   all pairs from the raw frame: any pbc_flags, any cutoff; tgt / ref: device index lists (NULL = 0..n-1)
 *   vmd_hip_within_pencil  the cell walk over the cell-sorted copies of both sets (K1, same grid, same boxes and flags, the pencil reach set
 *                          by vmd_hip_set_pencil_reach); the grid edge must be >= rmax as for vmd_hip_rdf_pencil.  Does nothing but the
 *                          zeroing when *skip_flag != 0 (see vmd_hip_cells_build_pencil).
 *   vmd_hip_within_to_float  out[b] = (float)counts[b] (does nothing when *skip_flag != 0) */
int vmd_hip_within_brute(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                         const float* boxes, uint32_t pbc_flags, int B,
                         const int32_t* tgt, int ntgt, const int32_t* ref, int nref,
                         float rmin, float rmax, int closed, uint32_t* count_out);
int vmd_hip_within_pencil(void* stream, const float* sorted_ref, const uint32_t* cell_start_ref, int nref, int nref_pad,
                          const float* sorted_tgt, const uint32_t* cell_start_tgt, int ntgt, int ntgt_pad,
                          const float* boxes, int B, vmd_grid_t grid, float rmin, float rmax, int closed,
                          uint32_t pbc_flags, uint32_t* count_out, const uint32_t* skip_flag);
int vmd_hip_within_to_float(void* stream, const uint32_t* counts, int B, float* out, const uint32_t* skip_flag);

/* K7: a within() shell as an rdf() argument, DESIGN 1.7.  The walks of K6 with one more product - WHICH entries are in:
 *   vmd_hip_within_brute_flags   flags_out u8[B][ntgt] in list order (1 = in the shell); count_out as vmd_hip_within_brute
 *   vmd_hip_within_pencil_flags  flags_out u8[B][ntgt_pad], one byte per SORTED position of the target copy (positions < ntgt are written);
 *                                pen_hits_out u32[B][ny*nz + 1], the hits of every pencil (the last entry is scratch); count_out as
 *                                vmd_hip_within_pencil.  Nothing but the zeroing of count_out happens when *skip_flag != 0
 *   vmd_hip_shell_compact        the flagged entries of (sorted, cell_start), in place order, become (sorted_hit f32[B][3][nsel_pad],
 *                                cell_start_hit u32[B][ncell+1]) on the same grid: a selection vmd_hip_rdf_pencil takes as it is.
 *                                pen_base u32[B][ny*nz + 1] is scratch (must not alias pen_hits).  Entries of sorted_hit beyond a frame's
 *                                population are left as they are: give the buffer the slack and the finite contents of a parent's rows.
 *                                Does nothing but the prefix when *skip_flag != 0
 *   vmd_hip_rdf_brute_masked     vmd_hip_rdf_brute with optional per-frame masks u8[B][nref] / u8[B][ntgt] (NULL = every entry): an entry
 *                                whose byte is 0 takes no part in that frame.  B <= 65535 */
int vmd_hip_within_brute_flags(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                               const float* boxes, uint32_t pbc_flags, int B,
                               const int32_t* tgt, int ntgt, const int32_t* ref, int nref,
                               float rmin, float rmax, int closed, uint32_t* count_out, uint8_t* flags_out);
int vmd_hip_within_pencil_flags(void* stream, const float* sorted_ref, const uint32_t* cell_start_ref, int nref, int nref_pad,
                                const float* sorted_tgt, const uint32_t* cell_start_tgt, int ntgt, int ntgt_pad,
                                const float* boxes, int B, vmd_grid_t grid, float rmin, float rmax, int closed,
                                uint32_t pbc_flags, uint32_t* count_out, const uint32_t* skip_flag,
                                uint8_t* flags_out, uint32_t* pen_hits_out);
int vmd_hip_shell_compact(void* stream, const uint8_t* flags, const uint32_t* pen_hits, uint32_t* pen_base,
                          const float* sorted, const uint32_t* cell_start, int nsel_pad, int B, vmd_grid_t grid,
                          float* sorted_hit, uint32_t* cell_start_hit, const uint32_t* skip_flag);
int vmd_hip_rdf_brute_masked(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                             const float* boxes, uint32_t pbc_flags, int B,
                             const int32_t* ref, int nref, const uint8_t* ref_mask, const int32_t* tgt, int ntgt,
                             const uint8_t* tgt_mask, float rmin, float rmax, int nbins, uint64_t* counts);

/* K8: a within() shell's members BY ATOM, DESIGN 1.8.  mask_out is u8[B][mask_stride] indexed by atom index: mask_out[b][tgt[t]] = 1 when
 * entry t of the target list is in the shell of frame b, else 0 - the membership of vmd_hip_within_brute_flags, bit for bit.  The calls write
 * the bytes of the atoms of `tgt` and nothing else: whoever allocates the mask zeroes it once if bytes of other atoms are ever read (the
 * evaluator does, for a target list that lost its reference atoms to spec_within_exclude_ref); mask_stride must exceed every index of tgt.
 * count_out u32[B] (zeroed by the call) = the per-frame populations.  B <= 65535.
 *   vmd_hip_within_atoms        the cell walk with only the REFERENCE set cell-sorted (K1; `boxes`, pbc_flags and grid those of its build, the
 *                               pencil reach set by vmd_hip_set_pencil_reach): one lane per list entry reads the raw frame, wraps the atom and
 *                               finds its pencil as a cell build would.  Nothing but the zeroing of count_out happens when *skip_flag != 0
 *   vmd_hip_within_brute_atoms  all pairs from the raw frame (any cell, any cutoff), vmd_hip_within_brute_flags with the bytes in atom order
 *   vmd_hip_sdf_scatter_masked  vmd_hip_sdf_scatter for a shell target: a target atom whose mask byte of frame b is 0 takes no part in frame b;
 *                               exclusion rule, arithmetic and atomics are vmd_hip_sdf_scatter's.  Always the index-list / progression kernel
 *                               (no atom_tag, none of the tuning variants).  Does nothing when *skip_flag != 0 */
int vmd_hip_within_atoms(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                         const float* boxes, uint32_t pbc_flags, int B, const int32_t* tgt, int ntgt,
                         const float* sorted_ref, const uint32_t* cell_start_ref, int nref, int nref_pad, vmd_grid_t grid,
                         float rmin, float rmax, int closed, uint32_t* count_out, uint8_t* mask_out, size_t mask_stride,
                         const uint32_t* skip_flag);
int vmd_hip_within_brute_atoms(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                               const float* boxes, uint32_t pbc_flags, int B,
                               const int32_t* tgt, int ntgt, const int32_t* ref, int nref,
                               float rmin, float rmax, int closed, uint32_t* count_out, uint8_t* mask_out, size_t mask_stride);
/* K9: and / or / not over up to four within() shells, DESIGN 1.9.  bits is u8[B][stride] indexed by atom index, clean (0) before the first
 * term pass of a batch; stride must exceed every index of tgt.  A term pass tests the entries of `tgt` whose byte v has bit v of `live` set
 * against ONE term's reference set - the membership of vmd_hip_within_brute_atoms, bit for bit - and ORs 1 << term into the byte of a hit;
 * every other entry does no work and keeps its byte.  live = 0xffff tests every entry.  Nothing happens when *skip_flag != 0.
 *   vmd_hip_within_atoms_expr   the cell walk of vmd_hip_within_atoms over the cell-sorted copy of the term's reference set
 *   vmd_hip_within_brute_expr   all pairs from the raw frame (any cell, any cutoff)
 *   vmd_hip_shell_expr_finish   mask_out[b][tgt[t]] = bit bits[b][tgt[t]] of `truth` (the layout of K8's masks; bytes of other atoms are not
 *                               written), count_out u32[B] (zeroed by the call) = the members per frame.  term < 4, truth and live < 2^16 */
int vmd_hip_within_atoms_expr(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                              const float* boxes, uint32_t pbc_flags, int B, const int32_t* tgt, int ntgt,
                              const float* sorted_ref, const uint32_t* cell_start_ref, int nref, int nref_pad, vmd_grid_t grid,
                              float rmin, float rmax, int closed, int term, uint32_t live, uint8_t* bits, size_t stride,
                              const uint32_t* skip_flag);
int vmd_hip_within_brute_expr(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                              const float* boxes, uint32_t pbc_flags, int B,
                              const int32_t* tgt, int ntgt, const int32_t* ref, int nref,
                              float rmin, float rmax, int closed, int term, uint32_t live, uint8_t* bits, size_t stride,
                              const uint32_t* skip_flag);
int vmd_hip_shell_expr_finish(void* stream, int B, const int32_t* tgt, int ntgt, const uint8_t* bits, uint32_t truth,
                              uint8_t* mask_out, size_t stride, uint32_t* count_out, const uint32_t* skip_flag);
int vmd_hip_sdf_scatter_masked(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                               const float* boxes, uint32_t pbc_flags, int B,
                               const int32_t* structs, int K, int m, const float* R32, const float* c32,
                               const int32_t* tgt, const int8_t* owner, int ntgt, float extent, int dim, uint64_t* volume,
                               const float* group, int tgt_first, int tgt_stride, int unowned,
                               const uint8_t* mask, size_t mask_stride, const uint32_t* skip_flag);

/* K12: hydrogen bonds, DESIGN 1.14.  A bond is one (donor pair j, acceptor entry k) combination: D = don[j], H = hyd[j], A = accl[k] at
 * 0 <= d(D, A) < r_da (closed != 0: <= r_da; the pair distance of K6), A neither D nor H by atom index, and the D-H...A angle at least
 * angle_min: with h = the minimum image of H - D from the raw frame, e the delta of the distance test, u = -h, v = -e - h:
 * u.u > 0, v.v > 0, u.v <= 0 and (u.v)^2 >= c2 (u.u v.v), c2 = fl(cos^2(angle_min)); every operation fp32, separately rounded.
 * Outputs: count_out u32[B] (zeroed by the call), the bonds of every frame; acc u64[npairs + nacc + 1], ADDED to: row j the bonds pair j
 * donated, row npairs + k the bonds entry k accepted.  Acceptor entries whose wrapped coordinates coincide bit for bit in a frame all
 * answer as the lowest of them (D-HB-COINCIDENT).  Nothing happens when *skip_flag != 0.  B <= 65535.
 *   vmd_hip_sorted_atoms  the identity of a cell-sorted copy (K1): ident_out u32[B][nsel_pad], slot -> the lowest list entry t whose wrapped
 *                         coordinates are the slot's, bit for bit; boxes are the GRID's, as the build took them
 *   vmd_hip_hbond_atoms   the cell walk of K8 over the cell-sorted copy of the acceptors, one lane per donor pair, every hit visited;
 *                         grid_boxes: the grid's; frame_boxes: the frames' own (the hydrogen's image)
 *   vmd_hip_hbond_brute   all pairs from the raw frame (any cell, any cutoff); canon: scratch, u32[B][nacc]
 *   vmd_hip_hbond_list    ONE frame by all pairs: list u32[list_cap][2] = {j, list position k} of the first list_cap bonds found (in no order;
 *                         the entry that answers for k is canon[k]), *list_count (device, zeroed by the call) = the bonds; nothing is
 *                         accumulated
 *   vmd_hip_hbond_finish  out[b] = (float)counts[b], *frames_row += B */
int vmd_hip_sorted_atoms(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags,
                         int B, const int32_t* sel, int nsel, const float* sorted, const uint32_t* cell_start, int nsel_pad, vmd_grid_t grid,
                         uint32_t* ident_out, const uint32_t* skip_flag);
int vmd_hip_hbond_atoms(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* grid_boxes,
                        const float* frame_boxes, uint32_t pbc_flags, int B, const int32_t* don, const int32_t* hyd, int npairs,
                        const int32_t* accl, int nacc, const float* sorted_acc, const uint32_t* cell_start_acc, int nacc_pad,
                        const uint32_t* ident, vmd_grid_t grid, float r_da, float c2, int closed, uint32_t* count_out, uint64_t* acc,
                        const uint32_t* skip_flag);
int vmd_hip_hbond_brute(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags,
                        int B, const int32_t* don, const int32_t* hyd, int npairs, const int32_t* accl, int nacc, uint32_t* canon,
                        float r_da, float c2, int closed, uint32_t* count_out, uint64_t* acc, const uint32_t* skip_flag);
int vmd_hip_hbond_list(void* stream, const float* xyz, size_t row_stride, const float* box, uint32_t pbc_flags, const int32_t* don,
                       const int32_t* hyd, int npairs, const int32_t* accl, int nacc, uint32_t* canon, float r_da, float c2, int closed,
                       uint32_t* list, uint32_t list_cap, uint32_t* list_count);
int vmd_hip_hbond_finish(void* stream, const uint32_t* counts, int B, float* out, uint64_t* frames_row, const uint32_t* skip_flag);

/* K13: solvent-accessible surface area by Shrake-Rupley, DESIGN 1.15.  Measured entry i (atom meas[i], R_i = r_meas[i]) carries the npoints
 * points R_i u_k of `points` f32[npoints][3] (1 <= npoints <= 256); n_i = the points inside no neighbour's sphere.  Environment entry j
 * (atom envl[j], R_j = r_env[j]; entries whose wrapped coordinates coincide bit for bit answer as the lowest of them, with its atom and its
 * R) is a neighbour iff 0 <= d < r_cut (closed != 0: <= r_cut; the pair distance of K6, e its delta, d2 the value it compared),
 * d2 < (R_i + R_j)^2 and its atom is not i's; it buries point k iff (u_kx e_x + u_ky e_y) + u_kz e_z < ((R_j R_j - R_i R_i) - d2) / (R_i + R_i).
 * fp32, every operation separately rounded.  rmax_env >= every r_env[j]; r_cut >= R_i + R_j for every pair.
 * Outputs: total_out u64[B] (zeroed by the call) = sum of n_i weight[i]; acc u64[nmeas + 1], ADDED to: row i += n_i.  Nothing happens when
 * *skip_flag != 0.  B <= 65535.
 *   vmd_hip_sasa_atoms   the cell walk of K8 over the cell-sorted copy of the environment (ident: vmd_hip_sorted_atoms' table of it), one
 *                        lane per measured entry
 *   vmd_hip_sasa_brute   all pairs from the raw frame (any cell, any cutoff); canon: scratch, u32[B][nenv]
 *   vmd_hip_sasa_list    ONE frame by all pairs: counts_out u32[nmeas] = n_i; nothing is accumulated
 *   vmd_hip_sasa_finish  out[b] = (float)(totals[b] * 2^-20), *frames_row += B */
#define VMD_SASA_POINTS_MAX 256
int vmd_hip_sasa_atoms(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* grid_boxes, uint32_t pbc_flags,
                       int B, const int32_t* meas, int nmeas, const int32_t* envl, int nenv, const float* sorted_env,
                       const uint32_t* cell_start_env, int nenv_pad, const uint32_t* ident, vmd_grid_t grid, const float* r_meas,
                       const float* r_env, float rmax_env, const uint32_t* weight, const float* points, int npoints, float r_cut, int closed,
                       uint64_t* total_out, uint64_t* acc, const uint32_t* skip_flag);
int vmd_hip_sasa_brute(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags, int B,
                       const int32_t* meas, int nmeas, const int32_t* envl, int nenv, uint32_t* canon, const float* r_meas, const float* r_env,
                       float rmax_env, const uint32_t* weight, const float* points, int npoints, float r_cut, int closed, uint64_t* total_out,
                       uint64_t* acc, const uint32_t* skip_flag);
int vmd_hip_sasa_list(void* stream, const float* xyz, size_t row_stride, const float* box, uint32_t pbc_flags, const int32_t* meas, int nmeas,
                      const int32_t* envl, int nenv, uint32_t* canon, const float* r_meas, const float* r_env, float rmax_env,
                      const float* points, int npoints, float r_cut, int closed, uint32_t* counts_out);
int vmd_hip_sasa_finish(void* stream, const uint64_t* totals, int B, float* out, uint64_t* frames_row, const uint32_t* skip_flag);

/* K14: residue contact maps, DESIGN 1.16.  The list `ent` (nent atoms) with `grp` (the group of every entry, 0 <= grp < ngroups) is walked
 * against ITSELF.  Groups g < h with h - g >= min_sep are in contact in frame b when an entry acting for g and an entry acting for h stand at
 * 0 <= d < r_cut (closed != 0: <= r_cut; the pair distance of K6); an entry acts for the group of the lowest list entry whose wrapped
 * coordinates coincide with its own bit for bit (D-CT-COINCIDENT).  bits: u32[B][W], W = ceil(P / 32), P = ngroups (ngroups - 1) / 2: bit
 * p & 31 of word p >> 5 is pair p = g (2 ngroups - g - 1) / 2 + (h - g - 1).  Nothing happens when *skip_flag != 0.  B <= 65535,
 * 2 <= ngroups <= 2048.
 *   vmd_hip_contact_atoms   the cell walk of K8 over the cell-sorted copy of the list, one lane per entry, every hit visited; bits are
 *                           cleared by the call.  ident: vmd_hip_sorted_atoms' table of the copy.  lds_rows != 0: a block ORs its hits
 *                           into LDS bit rows of the groups its entries act for and flushes the nonzero words (the same bits)
 *   vmd_hip_contact_brute   all pairs from the raw frame (any cell, any cutoff), the upper triangle of the entry pairs; bits are cleared by
 *                           the call; canon: scratch, u32[B][nent]
 *   vmd_hip_contact_finish  bits -> results: acc[p] += the frames of the B with bit p set (acc u64[P + 1], owned by this launch: a plain
 *                           add), acc[P] += B; out_count[b] = (float)popcount(row b); with nnative > 0 (native: u32[nnative] pair indices)
 *                           out_q[b] = (float)n_b / (float)nnative.  counts: scratch u32[2 B] */
int vmd_hip_contact_atoms(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* grid_boxes, uint32_t pbc_flags,
                          int B, const int32_t* ent, const int32_t* grp, int nent, int ngroups, uint32_t min_sep, const float* sorted,
                          const uint32_t* cell_start, int nent_pad, const uint32_t* ident, vmd_grid_t grid, float r_cut, int closed,
                          int lds_rows, uint32_t* bits, const uint32_t* skip_flag);
int vmd_hip_contact_brute(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags,
                          int B, const int32_t* ent, const int32_t* grp, int nent, int ngroups, uint32_t min_sep, uint32_t* canon,
                          float r_cut, int closed, uint32_t* bits, const uint32_t* skip_flag);
int vmd_hip_contact_finish(void* stream, const uint32_t* bits, int B, int ngroups, const uint32_t* native, int nnative, uint32_t* counts,
                           float* out_count, float* out_q, uint64_t* acc, const uint32_t* skip_flag);

/* K15: connected clusters of groups, DESIGN 1.17.  The list `ent` (nent atoms) with `grp` (the group of every entry, 0 <= grp < ngroups,
 * every group named) is walked against ITSELF.  Groups g != h are bonded in frame b when an entry of g and an entry of h stand at
 * 0 <= d < r_cut (closed != 0: <= r_cut; the pair distance of K6); the clusters are the connected components over all ngroups groups
 * (D-CL-GEOMETRIC: the lane's group from the list, a hit's through the identity table; the components are the same).  parent: u32[B][ngroups],
 * a lock-free union-find preset by the call to parent[g] = g; a root is hooked under a lower root only, so a component's final root is its
 * lowest group.  Nothing happens when *skip_flag != 0.  B <= 65535, 1 <= ngroups <= 2^24.
 *   vmd_hip_cluster_atoms   the cell walk of K8 over the cell-sorted copy of the list, one lane per entry, every hit of another group a
 *                           union.  ident: vmd_hip_sorted_atoms' table of the copy.  skip_same != 0: a lane skips the hits that repeat the
 *                           group it joined last (the same components)
 *   vmd_hip_cluster_brute   all pairs from the raw frame (any cell, any cutoff), the upper triangle of the entry pairs
 *   vmd_hip_cluster_finish  parent -> results: root[b][g] = the label of group g (its cluster's lowest group), size[b][r] = the groups
 *                           under root r (root, size: u32[B][ngroups]); acc[s - 1] += the clusters of s groups over the B frames,
 *                           acc[ngroups] += B (acc u64[ngroups + 1]); out_count[b] = (float)clusters, out_largest[b] = (float)largest size.
 *                           acc, out_count, out_largest may each be NULL.  counts: scratch u32[2 B].  wave_singles != 0: the clusters of
 *                           one group go to acc[0] as one add per wave (the same record) */
int vmd_hip_cluster_atoms(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* grid_boxes, uint32_t pbc_flags,
                          int B, const int32_t* ent, const int32_t* grp, int nent, int ngroups, const float* sorted,
                          const uint32_t* cell_start, int nent_pad, const uint32_t* ident, vmd_grid_t grid, float r_cut, int closed,
                          int skip_same, uint32_t* parent, const uint32_t* skip_flag);
int vmd_hip_cluster_brute(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags,
                          int B, const int32_t* ent, const int32_t* grp, int nent, int ngroups, float r_cut, int closed, uint32_t* parent,
                          const uint32_t* skip_flag);
int vmd_hip_cluster_finish(void* stream, const uint32_t* parent, uint32_t* root, uint32_t* size, int B, int ngroups, uint32_t* counts,
                           float* out_count, float* out_largest, uint64_t* acc, int wave_singles, const uint32_t* skip_flag);

/* K16: mean-squared displacement over lag times.  The position table has rows of 3 n + 9 floats: x[n], y[n], z[n] of the n
 * listed atoms as the frame holds them, then the frame's cell {L, 1/L, tilts} with L = 1/L = 0 on an axis that is not periodic
 * (its flag is clear in pbc_flags, or the frame's own edge is not positive).
 *   vmd_hip_msd_gather  rows f32[B][3 n + 9] of a batch; B <= 65535
 *   vmd_hip_msd_unwrap  counts i32[F][3][n], one word per axis: the image counts of the F consecutive rows at `rows`, 0 in the first, by the
 *                       SPEC S3 comparison under the later frame's cell (D-MSD-UNWRAP); an axis with L = 0 keeps its count
 *   vmd_hip_msd_lags    sums u64[max_lag + 1][4] are ADDED to: per lag tau the squared displacements along x, y, z in 2^-20 A^2 quanta,
 *                       q = (u64)((d * d) * 2^20) with d = (x(t + tau) - x(t)) + (float)(n(t + tau) - n(t)) * L(t + tau) in fp32, summed over
 *                       the origins t = 0, origin_stride, .. with t + tau < F and over the atoms, and the number of terms (origins x n).
 *                       0 <= max_lag < F, origin_stride >= 1, F <= 65535 * 32.  Integer sums: the same whatever the launch shape
 *   vmd_hip_msd_tile    the atoms, origin frames and lags a block of vmd_hip_msd_lags takes (the size edges of a test) */
#define VMD_MSD_MAX_ATOMS 0x0fffffff
#define VMD_MSD_CELL_FLOATS 9
int vmd_hip_msd_gather(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags, int B,
                       const int32_t* idx, int n, float* rows);
int vmd_hip_msd_unwrap(void* stream, const float* rows, int F, int n, int32_t* counts);
int vmd_hip_msd_lags(void* stream, const float* rows, const int32_t* counts, int F, int n, int max_lag, int origin_stride, uint64_t* sums);
int vmd_hip_msd_tile(int* atoms, int* origins, int* lags);

/* dst[i] += mult * src[i] (u64): one pair pass feeding several histograms; does nothing when *skip_flag != 0 */
int vmd_hip_axpy_u64(void* stream, uint64_t* dst, const uint64_t* src, size_t n, uint64_t mult, const uint32_t* skip_flag);
/* dst[i] += src[i] (u64): merges a frame block's partial accumulator into the totals */
int vmd_hip_add_u64(void* stream, uint64_t* dst, const uint64_t* src, size_t n);
/* u64 counters -> f32 values (values[i] = fl((float)counts[i] * scale); scale = 1: the raw counts of SPEC S5) + max reduction into
 * max_out[0] (device f32) */
int vmd_hip_counts_to_float(void* stream, const uint64_t* counts, size_t n, float* values, float* max_out, float scale);
/* K10: backbone phi / psi and the Ramachandran density.  One thread per (frame, segment): phi = dihedral(C[s-1], N[s], CA[s],
 * C[s]), psi = dihedral(N[s], CA[s], C[s], N[s+1]) with k_geom<4>'s arithmetic on raw positions, radians; a missing neighbour gives +0.
 * out f32[B][nseg][2] = {phi, psi}; link u8[nseg]: bit 0 has predecessor (segment s-1), bit 1 has successor (s+1).  B * nseg > 2^31 - 1
 * is refused. */
#define VMD_RAMA_DIM 512
#define VMD_RAMA_CLASSES 4
int vmd_hip_backbone_angles(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes,
                            uint32_t pbc_flags, int B, int nseg, const int32_t* n, const int32_t* ca, const int32_t* c,
                            const uint8_t* link, float* out);
/* bins rows [0, F) of `angles` (row r at angles + r * 2 * nseg) whose mask byte is non-zero (mask NULL: all); rama_class u8[nseg]: 0..3,
 * 255 = never binned; skip_ends: a segment that lacks a neighbour is not binned; a sample with phi == 0 && psi == 0 never is.
 * counts u64[512*512*4] (entry (y * 512 + x) * 4 + class) and sums u64[4] (NULL: not wanted) are ADDED to.  F * nseg > 2^31 - 1 is refused. */
int vmd_hip_rama_bin(void* stream, const float* angles, int F, const uint8_t* row_mask, int nseg, const uint8_t* rama_class,
                     const uint8_t* link, int skip_ends, uint64_t* counts, uint64_t* sums);
/* K11: per-frame secondary structure, three launches over one scratch block of vmd_hip_ss_scratch_words(B, nseg) u64 - four
 * bit matrices [B][nseg][ceil(nseg / 64)]: HB, its transpose, the parallel and the antiparallel bridges.  n / ca / c / o i32[nseg] (o: -1 =
 * the segment has no carbonyl oxygen), rng i32[nseg] the range of every segment, pro u8[nseg] 1 = proline, nbmask u64[ceil(nseg / 64)] bit
 * j = segment j has both neighbours in its range.  vmd_hip_ss_hbond fills HB and its transpose, vmd_hip_ss_bridges the bridge rows from
 * them, vmd_hip_ss_assign the class row cls f32[B][nseg] (codes 1..8) and the populations pop f32[B][9] from all four.  nseg above
 * VMD_SS_SEG_MAX, B * nseg * ceil(nseg / 64) > 2^31 - 1 and NULL arguments are refused before anything is launched. */
#define VMD_SS_SEG_MAX 16384
#define VMD_SS_CODES 9
size_t vmd_hip_ss_scratch_words(int B, int nseg);
int vmd_hip_ss_hbond(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags,
                     int B, int nseg, const int32_t* n, const int32_t* ca, const int32_t* c, const int32_t* o, const int32_t* rng,
                     const uint8_t* pro, const uint64_t* nbmask, uint64_t* scratch);
int vmd_hip_ss_bridges(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags,
                       int B, int nseg, const int32_t* n, const int32_t* ca, const int32_t* c, const int32_t* o, const int32_t* rng,
                       const uint8_t* pro, const uint64_t* nbmask, uint64_t* scratch);
int vmd_hip_ss_assign(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags,
                      int B, int nseg, const int32_t* n, const int32_t* ca, const int32_t* c, const int32_t* o, const int32_t* rng,
                      const uint8_t* pro, const uint64_t* nbmask, uint64_t* scratch, float* cls, float* pop);
/* 1: k_sdf_scatter reads the frame with non-temporal loads; returns the previous value */
int vmd_hip_set_sdf_nt(int on);
/* candidate columns (one target atom against the 64 reference atoms of a chunk: 64 candidate lanes) k_rdf_pencil has walked on the
 * current device since the counter was last reset; synchronises the device */
uint64_t vmd_hip_rdf_columns(int reset);
/* counts[0] += value on the device (closed-interval RDF: the self pairs a half-shell pass never visits) */
int vmd_hip_bump_u64(void* stream, uint64_t* p, uint64_t value);
/* the selection the NEXT vmd_hip_cells_* calls of this host thread sort is periodic: atom(t) = first + (t / m) * period + off[t % m], 1 <= m <= 4
 * (the O of every water: m = 1, period 3) - the kernels compute it instead of reading sel[t].  m = 0: read the list (the default). */
void vmd_hip_set_cells_sel_pattern(int m, int first, int period, const int* off);
/* an empty kernel named k_marker_timed_region: a profiled command marks where its timed region begins (bench.py, scripts/pmc_traffic.py) */
int vmd_hip_marker(void* stream);
/* DECISION(D-RDF-OPEN) as a switch: 1 = hit iff r_min <= d <= r_max in the pair kernels launched from now on; returns the old value */
int vmd_hip_set_rdf_closed(int on);
int vmd_hip_set_rdf_raw(int on);        /* vmd_hip_rdf_brute: positions enter the pair computation unwrapped, minimum image by rounding (oracle/SPEC.md D-WRAP flipped); per host thread; returns the previous value */

/* XTC coordinate blocks decompressed on the device (the compressed bytes cross PCIe, not the floats): one
 * thread per frame walks its bit stream (frames are independent, a stream is strictly sequential).
 *   raw     u8: the bit streams, frame b at raw + info[b].offset (64-byte aligned, >= 32 readable bytes behind each stream)
 *   info    one record per frame, host byte order
 *   xyz     out, frame layout as above, Angstrom: fl(fl(int * fl(1/precision)) * 10) like the host reader (vmd_xdr.cpp)
 *   status  u32[B] out: 0 ok, 1 corrupt stream, 2 not supported on the device (a packed triple whose value needs more than 64 bits) */
typedef struct vmd_xtc_frame_t {
    float    precision;
    int32_t  minint[3], maxint[3];
    int32_t  smallidx;
    uint64_t offset, nbytes;
} vmd_xtc_frame_t;
/* Frames stored as plain floats (TRR, DCD), DMA'd as they lie in the file: swap / scale / transpose into the frame layout above.
 * raw + info[b].offset[c] + 4 * stride * i = component c of atom i of frame b (4-byte aligned); scale is one fp32 multiply, skipped
 * when it is 1 (the host readers do the same: vmd_xdr.cpp trr_load, vmd_dcd.cpp dcd_load_frame). */
typedef struct vmd_f32_frame_t {
    uint64_t offset[3];
    uint32_t stride, flags;     /* flags: bit 0 = big-endian */
    float    scale;
    uint32_t reserved;
} vmd_f32_frame_t;
int vmd_hip_raw_f32_decode(void* stream, const unsigned char* raw, const vmd_f32_frame_t* info, int B, int natoms,
                           float* xyz, size_t frame_stride, size_t row_stride);

int vmd_hip_xtc_decode(void* stream, const unsigned char* raw, const vmd_xtc_frame_t* info, int B, int natoms,
                       float* xyz, size_t frame_stride, size_t row_stride, uint32_t* status);
/* the same result in two passes: k_xtc_index (one thread per frame) follows only flags and field widths and drops a checkpoint
 * at the first atom-group boundary at or after every `chunk` atoms (>= 64), k_xtc_chunks decodes all chunks of all frames in
 * parallel (one thread per chunk).  scratch: vmd_hip_xtc_scratch_bytes(B, natoms, chunk) device bytes, 8-byte aligned. */
size_t vmd_hip_xtc_scratch_bytes(int B, int natoms, int chunk);
int vmd_hip_xtc_decode_chunked(void* stream, const unsigned char* raw, const vmd_xtc_frame_t* info, int B, int natoms,
                               float* xyz, size_t frame_stride, size_t row_stride, uint32_t* status, int chunk, void* scratch);
/* the same result with one WAVE per frame (k_xtc_wave): the wave walks the group boundaries of its stream speculatively (lane k
 * tests the flag bit of the k-th next group; the stream window lives in VGPRs, no LDS allocation) and decodes 64 groups at a time,
 * one per lane.  Streams of 2^27 bytes and more are reported as status 2. */
int vmd_hip_xtc_decode_wave(void* stream, const unsigned char* raw, const vmd_xtc_frame_t* info, int B, int natoms,
                            float* xyz, size_t frame_stride, size_t row_stride, uint32_t* status);
/* Checkpoints: the decoder state at a tile boundary of a frame's stream (bit position, atom index, smallidx | run << 8).  A first
 * pass (use = 0) decodes as vmd_hip_xtc_decode_wave does and writes up to VMD_XTC_CK_MAX of them per frame (ck[b][.], nck[b]); a
 * later pass over the SAME frames (use = 1) splits every frame into that many independent sections - no walk is repeated, a frame
 * occupies as many SIMDs as it has sections.  ck: device, B x VMD_XTC_CK_MAX records; nck: device, B counters. */
#define VMD_XTC_CK_MAX 64
typedef struct vmd_xtc_ck_t {
    uint32_t pos, atom, state, reserved;
} vmd_xtc_ck_t;
int vmd_hip_xtc_decode_wave_ck(void* stream, const unsigned char* raw, const vmd_xtc_frame_t* info, int B, int natoms,
                               float* xyz, size_t frame_stride, size_t row_stride, uint32_t* status, int use,
                               vmd_xtc_ck_t* ck, uint32_t* nck);
/* ... and with GROUP RECORDS next to the checkpoints: use = 0 also leaves one 16-bit record per decoded group (rec: B x rec_stride,
 * rec_stride >= natoms; nrec: B counters, 0 = no records for the frame): the bits the group spans (10), its smallidx step + 1 (2), the
 * atoms of its run (4).  use = 1 decodes from them (k_xtc_records): no walk, every tile of 64 groups is placed by three wave-wide
 * prefix sums and decoded independently; a record that does not describe the group found at its place fails the frame (status 1). */
int vmd_hip_xtc_decode_wave_rec(void* stream, const unsigned char* raw, const vmd_xtc_frame_t* info, int B, int natoms,
                                float* xyz, size_t frame_stride, size_t row_stride, uint32_t* status, int use,
                                vmd_xtc_ck_t* ck, uint32_t* nck, uint16_t* rec, uint32_t* nrec, size_t rec_stride);
/* waves that share one frame in k_xtc_wave (each walks the whole stream and decodes every n-th tile of 64 groups); 0 = automatic
 * (enough to put ~4 waves on every SIMD of the chip); returns the previous value */
int vmd_hip_set_xtc_waves(int n);

/* synthetic water box (oracle S9 twin): fills frames [frame0, frame0+B) of a batch laid out as above */
int vmd_hip_synth_frames(void* stream, float* xyz, size_t frame_stride, size_t row_stride, int B, uint32_t frame0,
                         uint64_t seed, uint32_t n_atoms, uint32_t n_blob, float L, float sigma);

#ifdef __cplusplus
}
#endif
#endif
