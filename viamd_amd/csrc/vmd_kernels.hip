// viamd_amd/csrc/vmd_kernels.hip — hand-written gfx950 (CDNA4, wave64) kernels of the RDF / SDF / distance
// hot path + the thin C-ABI launch layer declared in include/vmd_hip.h.
//
// Arithmetic contract: oracle/SPEC.md (S2 wrap, S3 pair displacement, S4 binning, S5 alignment/scatter,
// S6 distances).  This file is compiled with -ffp-contract=off: the only fused operations are the explicit
// fmaf() calls the spec names, so integer results are bit-identical to the CPU restatement.
//
// Reference functions replaced (sources live in the empty submodule ext/mdlib):
//   md_spatial_hash build/query  -> k_cells_bin_sorted / k_cells_pen_scan / k_cells_pen_sort (two-level build; single-level builds
//                                   k_cells_fused, k_cells_split_*, k_cells_count / _scan / _scatter for what it does not take) + the
//                                   segment walk of k_rdf_pencil
//   rdf()                        -> k_rdf_pencil (periodic, grid) / k_rdf_brute (general)
//   sdf() + density volume       -> k_sdf_align (fp64 Horn/Jacobi) + k_sdf_scatter
//   distance*()                  -> k_distance_com / k_distance_minmax / k_distance_pair
//   angle() / dihedral()         -> k_geom<3> / k_geom<4>
//   shape_weights()              -> k_shape_moments + k_shape_finish (large sets) / k_shape_small (populations of small sets)
//   rmsd()                       -> k_rmsd_shift + k_rmsd_moments + k_rmsd_finish (large sets) / k_rmsd_small; the frame-0 pose by the same kernels
//   rmsf           -> rmsd's sums, k_rmsf_rotation, k_rmsf_accumulate (large sets) / k_rmsf_small
//   hydrogen bonds -> k_sorted_atoms + k_hbond_atoms (the cell walk) / k_canon_entries + k_hbond_brute (all pairs), k_hbond_finish
//   accessible area -> k_sorted_atoms + k_sasa_atoms (the cell walk) / k_canon_entries + k_sasa_brute (all pairs), k_sasa_finish
//   contact maps   -> k_sorted_atoms + k_contact_atoms (the cell walk) / k_canon_entries + k_contact_brute (all pairs),
//                                   k_contact_finish_rows / _frames / _out
//   clusters       -> k_cluster_init, k_sorted_atoms + k_cluster_atoms (the cell walk) / k_cluster_brute (all pairs),
//                                   k_cluster_finish_roots / _count / _out
//   msd over lag times -> k_msd_gather (the position table's rows of a batch), k_msd_unwrap + k_msd_lags (a query)
//
// What the property kernels (K3 alignment, K5 - K5d, K10 backbone, K11 secondary structure) share, each written once:
//   vmd_frames_t / vmd_frames()  the head of their parameter blocks, filled by one host function; vmd_frame(): frame b's rows and cell
//   vmd_com_t                    the fp64 centre of mass of vmd_set_com, k_sdf_align and k_sdf_ref_pose
//   vmd_bond / vmd_normal / vmd_dihedral   the bond vectors and the dihedral of k_geom, k_backbone_angles and k_ss_assign's bend
//   vmd_set_*                    shape_weights' and rmsd's reduction (rules 1 - 5): constants, block decode, context slice,
//                                wave / block / chunk sums, the fp64 cell (vmd_set_frame) and the atom load (vmd_set_load)
//
// Design notes (DESIGN.md has the long form):
//  * wave64 everywhere; a wave is the unit of work in the pair kernel (private LDS histogram + private LDS
//    hit queue per wave, no block barrier in the hot loop).
//  * i atoms live in lanes, j atoms are wave-uniform: their coordinates come through the scalar cache
//    (s_load) and feed VALU ops as SGPR operands, so the candidate filter is 7 VALU ops per pair.
//  * hits are compacted through the per-wave LDS queue so that sqrt + binning + ds_add run on full waves.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "vmd_hip.h"

#define VMD_WAVE 64
#define VMD_MAX_BINS 1024
#define VMD_QUEUE_CAP 384          // floats: < 64 pending + 4 undrained candidate columns of 64 (variant 2: < 64 + 64 pair entries in two
                                   // planes of 128 floats, drained after every pair-column), + the 64-entry slow stack
#define VMD_PAIR_B 128             // variant 2: float offset of the second value of a pair entry (at most 64 + 64 entries are ever pending)
#define VMD_JUNK 3.0e38f           // partner value of a pair entry that must never be counted: far beyond any r_max
#define VMD_FAR 1.0e18f            // coordinate of a padding lane: never within any cutoff, squares stay finite

// Wave-uniform read-only data (j coordinates, cell offsets, boxes) is read through the constant address space so
// that hipcc emits s_load (scalar cache, SGPR operands) instead of per-lane global_load.  Legal because those
// arrays are only written by earlier kernels.  (The SIMT emulator under tests/emu defines this to nothing.)
// wave-wide predicate mask straight from the compare (HIP's __ballot goes through a 0/1 VGPR and a second v_cmp)
#ifndef VMD_BALLOT
#define VMD_BALLOT(pred) __builtin_amdgcn_ballot_w64(pred)
#endif
// the value lane `lane` (wave-uniform) holds in v, as a wave-uniform value: one v_readlane_b32.  (The SIMT emulator defines its own.)
#ifndef VMD_READLANE_U32
#define VMD_READLANE_U32(v, lane) ((uint32_t)__builtin_amdgcn_readlane((int)(v), (int)(lane)))
#endif
// floor-to-int and fractional part in one instruction each (v_cvt_flr_i32_f32, v_fract_f32)
#ifndef VMD_NO_INLINE_ASM
__device__ __forceinline__ int vmd_floor_to_int(float t) { int b; asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(b) : "v"(t)); return b; }
__device__ __forceinline__ float vmd_fract(float t) { return __builtin_amdgcn_fractf(t); }
// keeps a wave-uniform value in a VGPR (a VOP3 instruction takes only one SGPR operand; without this the compiler
// re-materialises the second one with a v_mov in the inner loop)
__device__ __forceinline__ float vmd_in_vgpr(float v) { float r; asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "s"(v)); return r; }
#else
__device__ __forceinline__ int vmd_floor_to_int(float t) { return (int)floorf(t); }
__device__ __forceinline__ float vmd_fract(float t) { return t - floorf(t); }
__device__ __forceinline__ float vmd_in_vgpr(float v) { return v; }
#endif
#ifndef VMD_UNIFORM_AS
#define VMD_UNIFORM_AS __attribute__((address_space(4)))
#endif
typedef VMD_UNIFORM_AS const float vmd_cf32;
typedef VMD_UNIFORM_AS const uint32_t vmd_cu32;
typedef float vmd_f2 __attribute__((vector_size(8)));   // two fp32 lanes of one VGPR/SGPR pair (v_pk_*_f32)
typedef float vmd_f4 __attribute__((vector_size(16), aligned(4)));
// four consecutive wave-uniform floats at byte offset `off` (32-bit: s_load_dwordx4 sdst, sbase, soffset)
__device__ __forceinline__ vmd_f4 vmd_uniform_load4(vmd_cf32* base, unsigned off) {
    return *(VMD_UNIFORM_AS const vmd_f4*)((VMD_UNIFORM_AS const char*)base + off);
}

// ------------------------------------------------------------------------------------------------ helpers

// SPEC S2
// invL = fl(1.0f / L), computed once per frame on the host (IEEE division, identical to the device's)
__device__ __forceinline__ float vmd_wrap(float x, float L, float invL) {
    const float t = x * invL;
    const float f = floorf(t);
    float xw = fmaf(-f, L, x);
    if (xw < 0.0f) xw = xw + L;
    if (xw >= L) xw = xw - L;
    return xw;
}

__device__ __forceinline__ float vmd_d2(float dx, float dy, float dz) { return fmaf(dz, dz, fmaf(dy, dy, dx * dx)); }

// SPEC S3 by comparison (general kernels)
__device__ __forceinline__ float vmd_mi_cmp(float d, float L, float hL, bool pbc) {
    if (pbc) {
        const float s = d > hL ? L : (d < -hL ? -L : 0.0f);
        d = d - s;
    }
    return d;
}

// SPEC S5/S6 fp32 minimum image by rint
__device__ __forceinline__ float vmd_mi_rintf(float d, float L, float invL, bool pbc) {
    if (pbc) d = fmaf(-rintf(d * invL), L, d);
    return d;
}

__device__ __forceinline__ double vmd_mi_rint(double d, double L, bool pbc) {
    if (pbc) d = d - L * rint(d / L);
    return d;
}

// One frame's unit cell as the kernels see it.  boxes[b*9 + ...] = {Lx,Ly,Lz, 1/Lx,1/Ly,1/Lz, xy,xz,yz}; pbc bit 3 = triclinic
// (basis a = (x,0,0), b = (xy,y,0), c = (xz,yz,z), all three axes periodic; SPEC S3t).
#define VMD_BOX_STRIDE 9
#define VMD_PBC_TRICLINIC 8u
struct vmd_box_t {
    float Lx, Ly, Lz, iLx, iLy, iLz, xy, xz, yz;
    bool px, py, pz, tri;
};
__device__ __forceinline__ vmd_box_t vmd_load_box(const float* boxes, int b, uint32_t pbc) {
    const float* q = boxes + (size_t)VMD_BOX_STRIDE * b;
    vmd_box_t bx;
    bx.Lx = q[0]; bx.Ly = q[1]; bx.Lz = q[2]; bx.iLx = q[3]; bx.iLy = q[4]; bx.iLz = q[5]; bx.xy = q[6]; bx.xz = q[7]; bx.yz = q[8];
    bx.px = pbc & 1u; bx.py = pbc & 2u; bx.pz = pbc & 4u; bx.tri = pbc & VMD_PBC_TRICLINIC;
    return bx;
}
// The head of every property kernel's parameter block (K3, K5 - K5d, K10, K11): the batch's coordinates, frame b at xyz + b * frame_stride
// as three rows row_stride apart, and its cells.  vmd_frame is frame b as a kernel sees it.
struct vmd_frames_t {
    const float* xyz; size_t frame_stride; size_t row_stride;
    const float* boxes; uint32_t pbc; int B;
};
static inline vmd_frames_t vmd_frames(const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags, int B) {
    return vmd_frames_t{xyz, frame_stride, row_stride, boxes, pbc_flags, B};
}
struct vmd_frame_t { const float* x; const float* y; const float* z; vmd_box_t bx; };
__device__ __forceinline__ vmd_frame_t vmd_frame(const vmd_frames_t& f, int b) {
    vmd_frame_t v;
    v.x = f.xyz + (size_t)b * f.frame_stride;
    v.y = v.x + f.row_stride;
    v.z = v.y + f.row_stride;
    v.bx = vmd_load_box(f.boxes, b, f.pbc);
    return v;
}
// SPEC S3t: Cartesian -> fractional and back, fp32
__device__ __forceinline__ void vmd_frac(const vmd_box_t& b, float x, float y, float z, float& sx, float& sy, float& sz) {
    sz = z * b.iLz;
    sy = fmaf(-b.yz, sz, y) * b.iLy;
    sx = fmaf(-b.xz, sz, fmaf(-b.xy, sy, x)) * b.iLx;
}
__device__ __forceinline__ void vmd_cart(const vmd_box_t& b, float sx, float sy, float sz, float& dx, float& dy, float& dz) {
    dz = sz * b.Lz;
    dy = fmaf(b.yz, sz, sy * b.Ly);
    dx = fmaf(b.xz, sz, fmaf(b.xy, sy, sx * b.Lx));
}
// SPEC S3t wrap: fractional coordinates folded into [0,1), back to Cartesian; (ux,uy,uz) = s_k * L_k are the unsheared
// coordinates the cell grid bins by
__device__ __forceinline__ void vmd_wrap_tri(const vmd_box_t& b, float x, float y, float z, float& xw, float& yw, float& zw,
                                             float& ux, float& uy, float& uz) {
    float sx, sy, sz;
    vmd_frac(b, x, y, z, sx, sy, sz);
    sx = sx - floorf(sx); if (!(sx < 1.0f)) sx = 0.0f;
    sy = sy - floorf(sy); if (!(sy < 1.0f)) sy = 0.0f;
    sz = sz - floorf(sz); if (!(sz < 1.0f)) sz = 0.0f;
    ux = sx * b.Lx; uy = sy * b.Ly; uz = sz * b.Lz;
    zw = uz;
    yw = fmaf(b.yz, sz, uy);
    xw = fmaf(b.xz, sz, fmaf(b.xy, sy, ux));
}
// SPEC S3t lattice vector n = (nx, ny, nz) in Cartesian components
__device__ __forceinline__ void vmd_lattice_shift(float Lx, float Ly, float Lz, float xy, float xz, float yz, float nx, float ny, float nz,
                                                  float& shx, float& shy, float& shz) {
    shx = fmaf(nz, xz, fmaf(ny, xy, nx * Lx));
    shy = fmaf(nz, yz, ny * Ly);
    shz = nz * Lz;
}
// SPEC S3t pair on wrapped Cartesian positions: image by rounding the displacement in fractional space
__device__ __forceinline__ float vmd_pair_d2_tri(const vmd_box_t& b, float xi, float yi, float zi, float xj, float yj, float zj) {
    const float d0x = xi - xj, d0y = yi - yj, d0z = zi - zj;
    float sx, sy, sz;
    vmd_frac(b, d0x, d0y, d0z, sx, sy, sz);
    float shx, shy, shz;
    vmd_lattice_shift(b.Lx, b.Ly, b.Lz, b.xy, b.xz, b.yz, rintf(sx), rintf(sy), rintf(sz), shx, shy, shz);
    return vmd_d2(d0x - shx, d0y - shy, d0z - shz);
}
// the coordinates pair kernels work on: wrapped Cartesian (S2 per axis for orthorhombic / open cells, S3t for triclinic)
__device__ __forceinline__ void vmd_pair_coords(const vmd_box_t& b, float x, float y, float z, float& ox, float& oy, float& oz) {
    if (b.tri) { float ux, uy, uz; vmd_wrap_tri(b, x, y, z, ox, oy, oz, ux, uy, uz); return; }
    ox = b.px ? vmd_wrap(x, b.Lx, b.iLx) : x;
    oy = b.py ? vmd_wrap(y, b.Ly, b.iLy) : y;
    oz = b.pz ? vmd_wrap(z, b.Lz, b.iLz) : z;
}
// the displacement of a pair of such positions, (i - j) - shift, the shift of the SPEC S3 / S3t image (vmd_pair_d2_tri's operations) ...
__device__ __forceinline__ void vmd_pair_delta_general(const vmd_box_t& b, float xi, float yi, float zi, float xj, float yj, float zj,
                                                       float& dx, float& dy, float& dz) {
    if (b.tri) {
        const float d0x = xi - xj, d0y = yi - yj, d0z = zi - zj;
        float sx, sy, sz, shx, shy, shz;
        vmd_frac(b, d0x, d0y, d0z, sx, sy, sz);
        vmd_lattice_shift(b.Lx, b.Ly, b.Lz, b.xy, b.xz, b.yz, rintf(sx), rintf(sy), rintf(sz), shx, shy, shz);
        dx = d0x - shx; dy = d0y - shy; dz = d0z - shz;
        return;
    }
    dx = vmd_mi_cmp(xi - xj, b.Lx, 0.5f * b.Lx, b.px);
    dy = vmd_mi_cmp(yi - yj, b.Ly, 0.5f * b.Ly, b.py);
    dz = vmd_mi_cmp(zi - zj, b.Lz, 0.5f * b.Lz, b.pz);
}
// ... and its square: the one definition of a pair's squared distance
__device__ __forceinline__ float vmd_pair_d2_general(const vmd_box_t& b, float xi, float yi, float zi, float xj, float yj, float zj) {
    float dx, dy, dz;
    vmd_pair_delta_general(b, xi, yi, zi, xj, yj, zj, dx, dy, dz);
    return vmd_d2(dx, dy, dz);
}
// SPEC S5/S6 minimum image of a Cartesian displacement by rounding (fp32 / fp64)
__device__ __forceinline__ void vmd_mi3_rintf(const vmd_box_t& b, float& dx, float& dy, float& dz) {
    if (b.tri) {
        float sx, sy, sz;
        vmd_frac(b, dx, dy, dz, sx, sy, sz);
        sx = sx - rintf(sx); sy = sy - rintf(sy); sz = sz - rintf(sz);
        vmd_cart(b, sx, sy, sz, dx, dy, dz);
        return;
    }
    dx = vmd_mi_rintf(dx, b.Lx, b.iLx, b.px);
    dy = vmd_mi_rintf(dy, b.Ly, b.iLy, b.py);
    dz = vmd_mi_rintf(dz, b.Lz, b.iLz, b.pz);
}
__device__ __forceinline__ void vmd_mi3_rint(const vmd_box_t& b, double& dx, double& dy, double& dz) {
    if (b.tri) {
        double sz = dz / (double)b.Lz;
        double sy = (dy - (double)b.yz * sz) / (double)b.Ly;
        double sx = (dx - (double)b.xy * sy - (double)b.xz * sz) / (double)b.Lx;
        sx = sx - rint(sx); sy = sy - rint(sy); sz = sz - rint(sz);
        dz = sz * (double)b.Lz;
        dy = sy * (double)b.Ly + (double)b.yz * sz;
        dx = sx * (double)b.Lx + (double)b.xy * sy + (double)b.xz * sz;
        return;
    }
    dx = vmd_mi_rint(dx, (double)b.Lx, b.px);
    dy = vmd_mi_rint(dy, (double)b.Ly, b.py);
    dz = vmd_mi_rint(dz, (double)b.Lz, b.pz);
}

__device__ __forceinline__ int vmd_cell_coord(float v, float inv, int n) {
    int c = (int)(v * inv);
    c = c < 0 ? 0 : c;
    return c > n - 1 ? n - 1 : c;
}

__device__ __forceinline__ float vmd_wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float vmd_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float vmd_uniform(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
// The same two reductions for a full wave of 64 active lanes, as one wave-uniform value and without lane addresses: __shfl_xor is
// ds_bpermute_b32 behind a per-lane byte address (lane ^ o, clamped, times four - three VALU instructions per step that k_rdf_pencil
// recomputed for every work item, and six VGPRs held across its column loops); ds_swizzle_b32 carries the xor in its immediate (bit-mask
// mode: and 0x1f, or 0, xor o, inside each half of the wave), and lane 0 - the one vmd_uniform reads - takes the other half's result from
// lane 32 through one v_readlane.  min / max are exact: the order of the steps does not change the value.
#ifndef VMD_NO_INLINE_ASM
#define VMD_SWIZZLE_XOR(v, o) __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), ((o) << 10) | 0x1f))
__device__ __forceinline__ float vmd_wave64_min(float v) {
    v = fminf(v, VMD_SWIZZLE_XOR(v, 16)); v = fminf(v, VMD_SWIZZLE_XOR(v, 8)); v = fminf(v, VMD_SWIZZLE_XOR(v, 4));
    v = fminf(v, VMD_SWIZZLE_XOR(v, 2)); v = fminf(v, VMD_SWIZZLE_XOR(v, 1));
    return vmd_uniform(fminf(v, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32))));
}
__device__ __forceinline__ float vmd_wave64_max(float v) {
    v = fmaxf(v, VMD_SWIZZLE_XOR(v, 16)); v = fmaxf(v, VMD_SWIZZLE_XOR(v, 8)); v = fmaxf(v, VMD_SWIZZLE_XOR(v, 4));
    v = fmaxf(v, VMD_SWIZZLE_XOR(v, 2)); v = fmaxf(v, VMD_SWIZZLE_XOR(v, 1));
    return vmd_uniform(fmaxf(v, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32))));
}
// keeps the compiler from evaluating what depends on v before the branch that guards it (an empty volatile asm is not speculated)
__device__ __forceinline__ float vmd_pin(float v) { asm volatile("" : "+v"(v)); return v; }
#else
__device__ __forceinline__ float vmd_wave64_min(float v) { return vmd_uniform(vmd_wave_min(v)); }
__device__ __forceinline__ float vmd_wave64_max(float v) { return vmd_uniform(vmd_wave_max(v)); }
__device__ __forceinline__ float vmd_pin(float v) { return v; }
#endif
__device__ __forceinline__ unsigned vmd_lane_prefix(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// SPEC S4: bin of one squared distance, -1 when outside the open interval
struct vmd_binning_t {
    float rmin, rmax, inv_range, fnbins;
    int nbins;
    // fast path of vmd_bin_add: t' = fma(v_sqrt_f32(d2), fast_k, fast_c) approximates the spec's scaled distance to within
    // fast_delta/4; it is trusted when it lies at least fast_delta away from every integer (bin edge, and through bins 0 and
    // nbins-1 also from r_min / r_max); everything else takes the exact path
    float fast_k, fast_c, fast_half;   // fast_half = 0.5 - fast_delta
    float fast_far;                    // t' >= fast_far: beyond r_max by a whole bin, i.e. certainly not a hit (pair entries carry such partners)
    // the same test with fast_delta folded into the constant (r_min = 0 only, vmd_pop_hot0): t2 = fma(v_sqrt_f32(d2), fast_k, fast_delta) is
    // t' + delta, so "t' at least delta away from every integer" reads  fract(t2) > 2 delta  and floor(t2) is the bin - one compare instead of
    // add + compare, and no range test: t2 > 0 always, and t2 >= nbins (d > r_max, still below the padded cutoff) lands in a spare bin
    float fast_c2, fast_2d;            // fast_delta, 2 * fast_delta; fast_2d >= 1 (nothing is ever sure) when the fold does not apply
    int closed;                        // DECISION(D-RDF-OPEN) flipped: hit iff r_min <= d <= r_max.  Only vmd_bin_of looks at it: the fast path is
                                       // never trusted within delta of a bin edge, and d = r_min / r_max sit exactly on one
};
static thread_local int g_rdf_closed = 0;       // per host thread: set from the eval's spec right before that thread's launches (two evals with different specs on two threads must not race)
extern "C" int vmd_hip_set_rdf_closed(int on) { const int old = g_rdf_closed; g_rdf_closed = on ? 1 : 0; return old; }
static thread_local int g_rdf_raw = 0;          // k_rdf_brute: positions unwrapped, minimum image by rounding (DECISION D-WRAP flipped); per host thread like g_rdf_closed
extern "C" int vmd_hip_set_rdf_raw(int on) { const int old = g_rdf_raw; g_rdf_raw = on ? 1 : 0; return old; }
__host__ __device__ inline vmd_binning_t vmd_make_binning(float rmin, float rmax, int nbins, int closed = 0) {
    vmd_binning_t b;
    b.closed = closed;
    b.rmin = rmin; b.rmax = rmax; b.inv_range = 1.0f / (rmax - rmin); b.fnbins = (float)nbins; b.nbins = nbins;
    // error budget of t' = fma(v_sqrt(d2), k, c) against the spec value ((d - rmin) * inv_range) * nbins, in ulps of
    // T = rmax * inv_range * nbins (the largest intermediate): v_sqrt_f32 1 + fma 0.5 on our side, sqrtf 0.5 + subtraction
    // 0.5 + product 0.5 on the spec's (the factor nbins = 2^k is exact), the rounding of c = -rmin*k 0.5: 3.5 ulp
    // = 4.2e-7 * T.  delta = 6e-7 * T (5 ulp) + 2.5e-4 absolute head room.
    const float delta = 2.5e-4f + 6.0e-7f * rmax * b.inv_range * b.fnbins;
    b.fast_k = b.inv_range * b.fnbins;
    b.fast_c = -rmin * b.fast_k;
    b.fast_half = 0.5f - delta;
    b.fast_far = b.fnbins + 1.0f;                   // |t' - t| <= delta / 4 << 1: t' >= nbins + 1 implies d > r_max
    b.fast_c2 = delta; b.fast_2d = 2.0f * delta;
    if (!(delta < 0.25f)) { b.fast_half = -1.0f; b.fast_far = 3.0e38f; }      // degenerate range: nothing is ever "sure", exact path only
    if (!(delta < 0.25f) || rmin != 0.0f) b.fast_2d = 2.0f;                   // (v_fract_f32 < 1)
    return b;
}
__device__ __forceinline__ int vmd_bin_of(const vmd_binning_t& b, float d2) {
    const float d = sqrtf(d2);
    if (b.closed ? !(b.rmin <= d && d <= b.rmax) : !(b.rmin < d && d < b.rmax)) return -1;
    int bin = (int)(((d - b.rmin) * b.inv_range) * b.fnbins);
    bin = bin < 0 ? 0 : bin;
    return bin > b.nbins - 1 ? b.nbins - 1 : bin;
}

// ------------------------------------------------------------------------------------------------ K1: cell build

// A selection whose index list is periodic - atom(t) = first + (t / m) * period + off[t % m], m <= 4: "the O of every water" (m = 1, period 3),
// "the two H of every water" (m = 2), "every atom" - is not read from memory at all: the list costs 4 bytes per selected atom and frame (1.33 GB
// per 1 000 frames of the 1M-atom heavy-atom RDF, 4.8 % of the cell build's traffic) for something three integers say.  m = 0: read sel[t].
struct vmd_sel_pattern_t { int m, first, period; int off[4]; };
struct vmd_cells_params_t {
    const float* xyz; size_t frame_stride; size_t row_stride;
    const float* boxes; uint32_t pbc; const int32_t* sel; int nsel; int nsel_pad;
    vmd_grid_t grid;
    uint32_t* cell_count; uint32_t* rank; uint32_t* cell_start; float* sorted;
    float* aos;   // optional f32[B][nsel_pad][4] staging: scatter ONE 16-byte record per atom, k_cells_repack makes the SoA rows
    vmd_sel_pattern_t pat;
};

__device__ __forceinline__ int vmd_sel_atom(const vmd_cells_params_t& p, int t) {
    if (p.pat.m == 1) return p.pat.first + t * p.pat.period;
    if (p.pat.m > 1) { const int q = t / p.pat.m, r = t - q * p.pat.m; return p.pat.first + q * p.pat.period + p.pat.off[r]; }
    return p.sel ? p.sel[t] : t;
}

__device__ __forceinline__ uint32_t vmd_cell_of(const vmd_cells_params_t& p, int b, int t, float& xw, float& yw, float& zw) {
    const int a = vmd_sel_atom(p, t);
    const float* fx = p.xyz + (size_t)b * p.frame_stride;
    const float* bq = p.boxes + (size_t)VMD_BOX_STRIDE * b;
    const float Lx = bq[0], Ly = bq[1], Lz = bq[2], iLx = bq[3], iLy = bq[4], iLz = bq[5];
    float ux, uy, uz;     // what the grid bins by: wrapped coordinate (periodic axis), offset from the batch's bounding box
                          // (open axis; L is then the box extent, slots 6..8 the origin), or s_k * L_k (triclinic cell)
    if (p.pbc & VMD_PBC_TRICLINIC) {
        vmd_box_t bx;
        bx.Lx = Lx; bx.Ly = Ly; bx.Lz = Lz; bx.iLx = iLx; bx.iLy = iLy; bx.iLz = iLz; bx.xy = bq[6]; bx.xz = bq[7]; bx.yz = bq[8];
        bx.px = bx.py = bx.pz = bx.tri = true;
        vmd_wrap_tri(bx, fx[a], fx[p.row_stride + a], fx[2 * p.row_stride + a], xw, yw, zw, ux, uy, uz);
    } else {
        const float x = fx[a], y = fx[p.row_stride + a], z = fx[2 * p.row_stride + a];
        if (p.pbc & 1u) { ux = xw = vmd_wrap(x, Lx, iLx); } else { xw = x; ux = x - bq[6]; }
        if (p.pbc & 2u) { uy = yw = vmd_wrap(y, Ly, iLy); } else { yw = y; uy = y - bq[7]; }
        if (p.pbc & 4u) { uz = zw = vmd_wrap(z, Lz, iLz); } else { zw = z; uz = z - bq[8]; }
    }
    const int cx = vmd_cell_coord(ux, (float)p.grid.nxf * iLx, p.grid.nxf);
    const int cy = vmd_cell_coord(uy, (float)p.grid.ny * iLy, p.grid.ny);
    const int cz = vmd_cell_coord(uz, (float)p.grid.nz * iLz, p.grid.nz);
    return (uint32_t)((cz * p.grid.ny + cy) * p.grid.nxf + cx);
}

// a scattered 4-byte store costs the L2 as much as a scattered 16-byte one: the sort writes ONE float4 record per atom and
// k_cells_repack turns the records into the SoA rows with coalesced traffic
typedef float vmd_f4a __attribute__((vector_size(16)));
__device__ __forceinline__ void vmd_store_aos(float* aos, size_t slot, float x, float y, float z) {
    const vmd_f4a v = {x, y, z, 0.0f};
    *(vmd_f4a*)(aos + 4 * slot) = v;
}
// one atom of the sorted copy at slot `pos` of frame b: ONE record of the staging buffer when the build has one, else the three SoA rows
__device__ __forceinline__ void vmd_store_sorted(const vmd_cells_params_t& p, int b, uint32_t pos, float x, float y, float z) {
    if (p.aos) { vmd_store_aos(p.aos, (size_t)b * p.nsel_pad + pos, x, y, z); return; }
    float* s = p.sorted + (size_t)b * 3 * p.nsel_pad;
    s[pos] = x; s[p.nsel_pad + pos] = y; s[2 * (size_t)p.nsel_pad + pos] = z;
}

// Hillis-Steele inclusive scan of one value per thread of an NT-thread block over the CALLER's part[NT] (no helper of the builds owns LDS:
// k_cells_pen_sort gives all of its to the dynamic part) -> the thread's inclusive value; the total stays readable in part[NT - 1]
template <int NT>
__device__ __forceinline__ uint32_t vmd_block_scan(uint32_t* part, int tid, uint32_t v) {
    part[tid] = v;
    __syncthreads();
    for (int o = 1; o < NT; o <<= 1) {
        const uint32_t u = tid >= o ? part[tid - o] : 0u;
        __syncthreads();
        part[tid] += u;
        __syncthreads();
    }
    return part[tid];
}
// thread tid of NT owns the contiguous stretch [beg, end) of a table of n entries (empty for the last threads of a short table)
struct vmd_stretch_t { int beg, end; };
template <int NT>
__device__ __forceinline__ vmd_stretch_t vmd_stretch(int n, int tid) {
    const int per = (n + NT - 1) / NT, beg = tid * per;
    return {beg, beg + per < n ? beg + per : n};
}
// exclusive prefix over a table of n entries, a stretch per thread: count(c) is entry c's population, start(c, first) takes its first slot
template <int NT, class Count, class Start>
__device__ __forceinline__ void vmd_stretch_scan(uint32_t* part, int n, int tid, Count count, Start start) {
    const vmd_stretch_t st = vmd_stretch<NT>(n, tid);
    uint32_t sum = 0;
    for (int c = st.beg; c < st.end; ++c) sum += count(c);
    uint32_t run = vmd_block_scan<NT>(part, tid, sum) - sum;
    for (int c = st.beg; c < st.end; ++c) { const uint32_t m = count(c); start(c, run); run += m; }
}

__global__ __launch_bounds__(256) void k_cells_repack(const float* __restrict__ aos, float* __restrict__ sorted, int nsel, int nsel_pad) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (t >= nsel) return;
    const vmd_f4a v = *(const vmd_f4a*)(aos + 4 * ((size_t)b * nsel_pad + t));
    float* s = sorted + (size_t)b * 3 * nsel_pad;
    s[t] = v[0];
    s[nsel_pad + t] = v[1];
    s[2 * (size_t)nsel_pad + t] = v[2];
}

// atoms per thread.  Measured on the 333k-atom selection of config 3: 4 independent gathers per thread are ~10 % SLOWER than
// 1 (the kernels are bound by scattered 4-byte write / atomic transactions, not by latency), so this stays at 1.
#define VMD_CELLS_ILP 1
__global__ __launch_bounds__(256) void k_cells_count(vmd_cells_params_t p) {
    const int t0 = blockIdx.x * (256 * VMD_CELLS_ILP) + threadIdx.x;
    const int b = blockIdx.y;
    uint32_t c[VMD_CELLS_ILP];
    float xw, yw, zw;
#pragma unroll
    for (int u = 0; u < VMD_CELLS_ILP; ++u) {
        const int t = t0 + 256 * u;
        c[u] = t < p.nsel ? vmd_cell_of(p, b, t, xw, yw, zw) : 0xffffffffu;
    }
#pragma unroll
    for (int u = 0; u < VMD_CELLS_ILP; ++u) {
        const int t = t0 + 256 * u;
        if (c[u] != 0xffffffffu) p.rank[(size_t)b * p.nsel + t] = atomicAdd(&p.cell_count[(size_t)b * (p.grid.ncell + 1) + c[u]], 1u);
    }
}

// one 1024-thread block per frame: exclusive prefix over the cell populations.  Round 6: chunks of 4 096 cells, four CONSECUTIVE cells per
// thread - the previous version gave every thread its own contiguous stretch of ncell / 1024 cells, i.e. 64 lanes reading 64 different cache
// lines per load: 0.80 ms per dispatch for the 30 000 cells x 334 frames of config 5's solute class (profiles/r06z3_*), 2.4 ms of its step
__global__ __launch_bounds__(1024) void k_cells_scan(const uint32_t* __restrict__ cell_count, uint32_t* __restrict__ cell_start,
                                                     int ncell) {
    __shared__ uint32_t part[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint32_t* cnt = cell_count + (size_t)b * (ncell + 1);
    uint32_t* out = cell_start + (size_t)b * (ncell + 1);
    uint32_t carry = 0;
    for (int base = 0; base < ncell; base += 4096) {
        const int c0 = base + 4 * tid;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = c0 + k < ncell ? cnt[c0 + k] : 0u;
        const uint32_t s = v[0] + v[1] + v[2] + v[3];
        uint32_t run = carry + vmd_block_scan<1024>(part, tid, s) - s;   // exclusive
        const uint32_t total = part[1023];
#pragma unroll
        for (int k = 0; k < 4; ++k) { if (c0 + k < ncell) out[c0 + k] = run; run += v[k]; }
        carry += total;
        __syncthreads();                         // part[] is rewritten by the next chunk
    }
    if (tid == 0) out[ncell] = carry;
}

__global__ __launch_bounds__(256) void k_cells_scatter(vmd_cells_params_t p) {
    const int t0 = blockIdx.x * (256 * VMD_CELLS_ILP) + threadIdx.x;
    const int b = blockIdx.y;
    float xw[VMD_CELLS_ILP], yw[VMD_CELLS_ILP], zw[VMD_CELLS_ILP];
    uint32_t pos[VMD_CELLS_ILP];
#pragma unroll
    for (int u = 0; u < VMD_CELLS_ILP; ++u) {
        const int t = t0 + 256 * u;
        pos[u] = 0xffffffffu;
        if (t < p.nsel) {
            const uint32_t c = vmd_cell_of(p, b, t, xw[u], yw[u], zw[u]);
            pos[u] = p.cell_start[(size_t)b * (p.grid.ncell + 1) + c] + p.rank[(size_t)b * p.nsel + t];
        }
    }
#pragma unroll
    for (int u = 0; u < VMD_CELLS_ILP; ++u) if (pos[u] != 0xffffffffu) vmd_store_sorted(p, b, pos[u], xw[u], yw[u], zw[u]);
}

// Fused build for grids whose cell table fits in LDS: ONE 1024-thread block per frame does count (LDS atomics) ->
// exclusive scan (in LDS) -> scatter (LDS cursors).  No global atomics, no rank array, no separate scan launch.
// LDS: (ncell + 1) counters + 1024 scan partials.
__global__ __launch_bounds__(1024) void k_cells_fused(vmd_cells_params_t p) {
    HIP_DYNAMIC_SHARED(uint32_t, s_dyn)
    uint32_t* s_cnt = s_dyn;                       // [ncell + 1]
    uint32_t* s_part = s_dyn + p.grid.ncell + 1;   // [1024]
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int ncell = p.grid.ncell;
    for (int c = tid; c <= ncell; c += 1024) s_cnt[c] = 0u;
    __syncthreads();
    float xw, yw, zw;
    for (int t = tid; t < p.nsel; t += 1024) atomicAdd(&s_cnt[vmd_cell_of(p, b, t, xw, yw, zw)], 1u);
    __syncthreads();
    // the counters become cursors (a stretch of ceil(ncell / 1024) cells per thread: the table is in LDS, there are no loads to coalesce)
    uint32_t* out = p.cell_start + (size_t)b * (ncell + 1);
    vmd_stretch_scan<1024>(s_part, ncell, tid, [&](int c) { return s_cnt[c]; }, [&](int c, uint32_t first) { s_cnt[c] = first; out[c] = first; });
    if (tid == 1023) out[ncell] = s_part[1023];
    __syncthreads();
    for (int t = tid; t < p.nsel; t += 1024) {
        const uint32_t c = vmd_cell_of(p, b, t, xw, yw, zw);
        vmd_store_sorted(p, b, atomicAdd(&s_cnt[c], 1u), xw, yw, zw);
    }
}

// Split build for selections too large for one block per frame: G blocks share a frame, each owns a contiguous slice of the
// selection.  count: LDS histogram of the slice -> global table [frame][g][cell]; scan: per frame, exclusive prefix over
// cells of the column sums + running offset over g (in place: the table becomes each block's first slot per cell);
// scatter: LDS cursors initialised from the table.  No global atomics, no rank array; the only scattered traffic is the
// 16-byte record store.  The order of atoms inside a cell differs from the other builds (it is arbitrary in all of them).
struct vmd_cells_split_t {
    vmd_cells_params_t c;
    uint32_t* table;     // [B][G][ncell]
    int G; int slice;    // atoms per block (multiple of 1024)
};
// block g's slice of the selection: [t0, t1)
__device__ __forceinline__ void vmd_slice(const vmd_cells_split_t& q, int g, int& t0, int& t1) {
    t0 = g * q.slice; t1 = t0 + q.slice < q.c.nsel ? t0 + q.slice : q.c.nsel;
}

__global__ __launch_bounds__(1024) void k_cells_split_count(vmd_cells_split_t q) {
    HIP_DYNAMIC_SHARED(uint32_t, s_dyn)
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int ncell = q.c.grid.ncell;
    for (int c = tid; c < ncell; c += 1024) s_dyn[c] = 0u;
    __syncthreads();
    int t0, t1; vmd_slice(q, g, t0, t1);
    float xw, yw, zw;
    for (int t = t0 + tid; t < t1; t += 1024) atomicAdd(&s_dyn[vmd_cell_of(q.c, b, t, xw, yw, zw)], 1u);
    __syncthreads();
    uint32_t* out = q.table + ((size_t)b * q.G + g) * ncell;
    for (int c = tid; c < ncell; c += 1024) out[c] = s_dyn[c];
}

__global__ __launch_bounds__(1024) void k_cells_split_scan(uint32_t* __restrict__ table, uint32_t* __restrict__ cell_start, int ncell, int G) {
    __shared__ uint32_t part[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    uint32_t* tb = table + (size_t)b * G * ncell;
    uint32_t* out = cell_start + (size_t)b * (ncell + 1);
    uint32_t carry = 0;
    // rows of 1024 consecutive cells: thread = cell, so every table access is coalesced
    for (int base = 0; base < ncell; base += 1024) {
        const int c = base + tid;
        uint32_t s = 0;
        if (c < ncell) for (int g = 0; g < G; ++g) s += tb[(size_t)g * ncell + c];
        const uint32_t incl = vmd_block_scan<1024>(part, tid, s);
        if (c < ncell) {
            uint32_t run = carry + incl - s;         // exclusive
            out[c] = run;
            for (int g = 0; g < G; ++g) { const uint32_t n = tb[(size_t)g * ncell + c]; tb[(size_t)g * ncell + c] = run; run += n; }
        }
        carry += part[1023];
        __syncthreads();                             // part[] is rewritten by the next row
    }
    if (tid == 0) out[ncell] = carry;
}

__global__ __launch_bounds__(1024) void k_cells_split_scatter(vmd_cells_split_t q) {
    HIP_DYNAMIC_SHARED(uint32_t, s_dyn)
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int ncell = q.c.grid.ncell;
    const uint32_t* first = q.table + ((size_t)b * q.G + g) * ncell;
    for (int c = tid; c < ncell; c += 1024) s_dyn[c] = first[c];
    __syncthreads();
    int t0, t1; vmd_slice(q, g, t0, t1);
    float xw, yw, zw;
    for (int t = t0 + tid; t < t1; t += 1024) {
        const uint32_t c = vmd_cell_of(q.c, b, t, xw, yw, zw);
        vmd_store_sorted(q.c, b, atomicAdd(&s_dyn[c], 1u), xw, yw, zw);
    }
}

// Two-level build (the default): the frame is read ONCE and the sorted SoA rows are written once, with one 16-byte record per
// atom in between - against two reads of the frame, a scattered AoS write and a repack pass in the builds above.
//   level 1, k_cells_bin: a block takes a slice of the selection, wraps the atoms, counts them per PENCIL in LDS (a pencil =
//     one row of nxf fine cells; there are only ny*nz of them, so the table is tiny whatever nxf is), reserves room in every
//     pencil's bucket with one global atomic per (block, pencil) and writes the records {x, y, z, fine cell} there: a block's
//     atoms of one pencil land next to each other, so the scattered writes are short runs, not single records.
//   level 2, k_cells_pen_sort: one block per (frame, pencil) pulls the pencil's bucket through LDS (counting sort by fine cell)
//     and writes its stretch of the sorted rows and of cell_start fully coalesced.
// Buckets have a fixed capacity per pencil (pen_off, measured on a few frames by the host with k_cells_bin in counting mode, plus
// head room); an atom that finds its bucket full raises *overflow, every consumer of the sorted copy (k_rdf_pencil,
// k_hist_reduce) then does nothing, and the host re-measures and repeats the batch.  The order of atoms inside a cell depends on
// the order of the atomics (it is arbitrary in every build; the histograms do not depend on it).
struct vmd_bin_params_t {
    vmd_cells_params_t c;            // frame, boxes, selection, grid (cell_count / rank / aos unused)
    const uint32_t* pen_off;         // [npen + 1] exclusive prefix of the bucket capacities (records), NULL in counting mode
    uint32_t* pen_count;             // [B][npen], zeroed before the launch: atoms per pencil
    float* bucket;                   // [B][pen_off[npen]][4], NULL in counting mode
    uint32_t* overflow;              // [1]
    uint32_t overflow_bit;           // what an overflowing build ORs into it: one bit per selection, so that the host widens the buckets of THAT
                                     // selection only (c5, 1 000 frames: the wandering blob overflowed three times and took the water selections'
                                     // margins - and with them the two-level build - down with it: 49 ms of cell build per step instead of 21)
    int npen; int total_cap;
    int rec3;                        // 1: 12-byte records {x, y, z} (the fine cell follows from x alone: x-periodic, non-triclinic cells)
};
#define VMD_BIN_ILP 4          // atoms per thread: 4096-atom slices (8 per thread: measured slower, profiles/r02d_ab.txt)
// The bucket record, the one place that knows its two formats: rec3 ? 12 bytes {x, y, z} : 16 bytes {x, y, z, fine cell}.  `bk` is the first
// record of a run (a frame's buckets start at the same float whichever the format: vmd_rec_run), i counts records from there.
template <class F>
__device__ __forceinline__ F* vmd_rec_run(F* bucket, int b, int total_cap, int rec3, uint32_t first) {
    return bucket + 4 * (size_t)b * total_cap + (size_t)(rec3 ? 3 : 4) * first;
}
__device__ __forceinline__ void vmd_rec_put(float* bk, int rec3, size_t i, float x, float y, float z, uint32_t cx) {
    if (rec3) {
        float* r = bk + 3 * i;
        r[0] = x; r[1] = y; r[2] = z;
    } else {
        const vmd_f4a v = {x, y, z, __int_as_float((int)cx)};
        *(vmd_f4a*)(bk + 4 * i) = v;
    }
}
// the fine cell alone: reads word 3 (16-byte records) or x (12-byte records: the cell follows from x exactly as vmd_cell_of computed it,
// inv_cx = (float)nxf * the frame's 1 / Lx), nothing else
__device__ __forceinline__ uint32_t vmd_rec_get_cell(const float* bk, int rec3, size_t i, float inv_cx, int nxf) {
    return rec3 ? (uint32_t)vmd_cell_coord(bk[3 * i], inv_cx, nxf) : (uint32_t)__float_as_int(bk[4 * i + 3]);
}
__device__ __forceinline__ uint32_t vmd_rec_get(const float* bk, int rec3, size_t i, float inv_cx, int nxf, float& x, float& y, float& z) {
    if (rec3) {
        const float* r = bk + 3 * i;
        x = r[0]; y = r[1]; z = r[2];
        return (uint32_t)vmd_cell_coord(x, inv_cx, nxf);
    }
    const vmd_f4a v = *(const vmd_f4a*)(bk + 4 * i);
    x = v[0]; y = v[1]; z = v[2];
    return (uint32_t)__float_as_int(v[3]);
}

// The head of level 1: the thread's VMD_BIN_ILP atoms of block g's slice, wrapped, with pencil, fine cell and rank among the block's atoms of
// that pencil (pen = 0xffffffff: no atom).  Zeroes the block's pencil counters s_cnt[npen] first; they are complete when it returns.
struct vmd_bin_atoms_t {
    float xw[VMD_BIN_ILP], yw[VMD_BIN_ILP], zw[VMD_BIN_ILP];
    uint32_t pen[VMD_BIN_ILP], cx[VMD_BIN_ILP], rank[VMD_BIN_ILP];
};
__device__ __forceinline__ void vmd_bin_head(const vmd_bin_params_t& q, uint32_t* s_cnt, int g, int b, int tid, vmd_bin_atoms_t& a) {
    const uint32_t nxf = (uint32_t)q.c.grid.nxf;
    for (int c = tid; c < q.npen; c += 1024) s_cnt[c] = 0u;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < VMD_BIN_ILP; ++u) {
        const int t = (g * VMD_BIN_ILP + u) * 1024 + tid;
        a.pen[u] = 0xffffffffu;
        if (t < q.c.nsel) {
            const uint32_t cell = vmd_cell_of(q.c, b, t, a.xw[u], a.yw[u], a.zw[u]);
            a.pen[u] = cell / nxf;
            a.cx[u] = cell - a.pen[u] * nxf;
        }
    }
#pragma unroll
    for (int u = 0; u < VMD_BIN_ILP; ++u) if (a.pen[u] != 0xffffffffu) a.rank[u] = atomicAdd(&s_cnt[a.pen[u]], 1u);
    __syncthreads();
}

__global__ __launch_bounds__(1024) void k_cells_bin(vmd_bin_params_t q) {
    HIP_DYNAMIC_SHARED(uint32_t, s_dyn)
    uint32_t* s_cnt = s_dyn;                 // [npen] atoms of this block per pencil, then the block's first slot in the bucket
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int npen = q.npen;
    vmd_bin_atoms_t a;
    vmd_bin_head(q, s_cnt, g, b, tid, a);
    uint32_t* gcount = q.pen_count + (size_t)b * npen;
    for (int c = tid; c < npen; c += 1024) {
        const uint32_t n = s_cnt[c];
        if (n) s_cnt[c] = atomicAdd(&gcount[c], n);
    }
    if (!q.bucket) return;                   // counting mode: the host only wants the populations
    __syncthreads();
    float* bk = vmd_rec_run(q.bucket, b, q.total_cap, q.rec3, 0u);
#pragma unroll
    for (int u = 0; u < VMD_BIN_ILP; ++u) {
        if (a.pen[u] == 0xffffffffu) continue;
        const uint32_t off = q.pen_off[a.pen[u]], cap = q.pen_off[a.pen[u] + 1] - off;
        const uint32_t slot = s_cnt[a.pen[u]] + a.rank[u];
        if (slot < cap) vmd_rec_put(bk, q.rec3, (size_t)(off + slot), a.xw[u], a.yw[u], a.zw[u], a.cx[u]);
        else atomicOr(q.overflow, q.overflow_bit);
    }
}

// k_cells_bin_sorted's scan of one value per thread of its 1024-thread block, over the caller's s_p[1024 + 16]: two block barriers against the
// twenty of vmd_block_scan.  A measured choice, as the block scan is k_cells_pen_sort's: the two are not to be merged.  -> inclusive value
__device__ __forceinline__ uint32_t vmd_wave_scan_1024(uint32_t* s_p, int tid, uint32_t sum, uint32_t& total) {
    const int lane = tid & 63, wave = tid >> 6;
    volatile uint32_t* vp = s_p;                             // lanes exchange through LDS between wave barriers: no caching in registers
    vp[tid] = sum;
    __builtin_amdgcn_wave_barrier();
    for (int o = 1; o < VMD_WAVE; o <<= 1) {                 // inclusive scan of the wave's 64 partials, through LDS
        const uint32_t v = lane >= o ? vp[tid - o] : 0u;
        __builtin_amdgcn_wave_barrier();
        vp[tid] = vp[tid] + v;
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == VMD_WAVE - 1) vp[1024 + wave] = vp[tid];
    __syncthreads();
    if (wave == 0) {                                         // the 16 wave totals (every lane of the wave walks the barriers)
        for (int o = 1; o < 16; o <<= 1) {
            const uint32_t v = (lane < 16 && lane >= o) ? vp[1024 + lane - o] : 0u;
            __builtin_amdgcn_wave_barrier();
            if (lane < 16) vp[1024 + lane] = vp[1024 + lane] + v;
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    total = s_p[1024 + 15];
    return s_p[tid] + (wave ? s_p[1024 + wave - 1] : 0u);
}

// Level 1 with a block-local sort (the default): k_cells_bin stores every record from the lane that wrapped the atom, i.e. a wave's 64
// records go to ~64 different buckets - one partial-line write transaction each.  Here the block first orders its 4 096 records by
// pencil in LDS (rank inside the pencil from the LDS counter, the pencil's first slot from a block scan of the counters), then
// consecutive lanes write consecutive records: a (block, pencil) run of ~14 records leaves as one or two coalesced stores.
// LDS: 3 tables of npen words + 1 040 scan words + 4 096 records of 4 (12-byte output) or 5 (16-byte output) words.
__global__ __launch_bounds__(1024) void k_cells_bin_sorted(vmd_bin_params_t q) {
    HIP_DYNAMIC_SHARED(uint32_t, s_dyn)
    const int npen = q.npen;
    const int rw = q.rec3 ? 4 : 5;             // words per LDS record: x, y, z, pencil (, fine cell)
    uint32_t* s_cnt = s_dyn;                   // [npen] atoms of this block per pencil
    uint32_t* s_off = s_dyn + npen;            // [npen] first LDS slot of the pencil's run
    uint32_t* s_gbase = s_dyn + 2 * npen;      // [npen] first slot of the run in the pencil's bucket
    uint32_t* s_p = s_dyn + 3 * npen;          // [1024 + 16] scan partials
    uint32_t* s_rec = s_p + 1040;              // [4096][rw]
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    vmd_bin_atoms_t a;
    vmd_bin_head(q, s_cnt, g, b, tid, a);
    // reserve the runs in the buckets, and scan the counters: every thread its stretch of them
    uint32_t* gcount = q.pen_count + (size_t)b * npen;
    const vmd_stretch_t st = vmd_stretch<1024>(npen, tid);
    uint32_t sum = 0;
    for (int c = st.beg; c < st.end; ++c) {
        const uint32_t n = s_cnt[c];
        s_gbase[c] = n ? atomicAdd(&gcount[c], n) : 0u;
        sum += n;
    }
    uint32_t ntot;
    uint32_t run = vmd_wave_scan_1024(s_p, tid, sum, ntot) - sum;
    for (int c = st.beg; c < st.end; ++c) { s_off[c] = run; run += s_cnt[c]; }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < VMD_BIN_ILP; ++u) {
        if (a.pen[u] == 0xffffffffu) continue;
        uint32_t* r = s_rec + (size_t)rw * (s_off[a.pen[u]] + a.rank[u]);
        r[0] = (uint32_t)__float_as_int(a.xw[u]); r[1] = (uint32_t)__float_as_int(a.yw[u]); r[2] = (uint32_t)__float_as_int(a.zw[u]); r[3] = a.pen[u];
        if (!q.rec3) r[4] = a.cx[u];
    }
    __syncthreads();
    float* bk = vmd_rec_run(q.bucket, b, q.total_cap, q.rec3, 0u);
    bool over = false;
    for (uint32_t t = tid; t < ntot; t += 1024) {
        const uint32_t* r = s_rec + (size_t)rw * t;
        const uint32_t pn = r[3];
        const uint32_t off = q.pen_off[pn], cap = q.pen_off[pn + 1] - off;
        const uint32_t slot = s_gbase[pn] + (t - s_off[pn]);
        if (slot < cap) vmd_rec_put(bk, q.rec3, (size_t)(off + slot), __int_as_float((int)r[0]), __int_as_float((int)r[1]), __int_as_float((int)r[2]), q.rec3 ? 0u : r[4]);
        else over = true;
    }
    if (over) atomicOr(q.overflow, q.overflow_bit);
}

// per frame: exclusive prefix of the (capacity-clamped) pencil populations = first sorted slot of every pencil
__global__ __launch_bounds__(256) void k_cells_pen_scan(const uint32_t* __restrict__ pen_count, const uint32_t* __restrict__ pen_off,
                                                        uint32_t* __restrict__ pen_start, int npen) {
    __shared__ uint32_t part[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint32_t* cnt = pen_count + (size_t)b * npen;
    uint32_t* out = pen_start + (size_t)b * (npen + 1);
    vmd_stretch_scan<256>(part, npen, tid,
                          [&](int c) { const uint32_t cap = pen_off[c + 1] - pen_off[c]; return cnt[c] < cap ? cnt[c] : cap; },
                          [&](int c, uint32_t first) { out[c] = first; });
    if (tid == 255) out[npen] = part[255];
}

struct vmd_pensort_params_t {
    const float* bucket; const uint32_t* pen_off; const uint32_t* pen_count; const uint32_t* pen_start;
    uint32_t* cell_start; float* sorted;
    int npen, nxf, ncell, nsel_pad, total_cap, cap_max;
    const float* boxes; int rec3;      // rec3: 12-byte records, the fine cell is recomputed from x exactly as vmd_cell_of computed it
};
__global__ __launch_bounds__(256) void k_cells_pen_sort(vmd_pensort_params_t q) {
    HIP_DYNAMIC_SHARED(uint32_t, s_dyn)
    uint32_t* s_cnt = s_dyn;                                  // [nxf]
    uint32_t* s_part = s_dyn + q.nxf;                         // [256] scan partials (no static LDS: the dynamic part may take it all)
    float* s_xyz = (float*)(s_dyn + q.nxf + 256);             // [3][cap_max]
    const int pen = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int nxf = q.nxf;
    const uint32_t off = q.pen_off[pen], cap = q.pen_off[pen + 1] - off;
    uint32_t n = q.pen_count[(size_t)b * q.npen + pen];
    n = n < cap ? n : cap;
    const uint32_t start = q.pen_start[(size_t)b * (q.npen + 1) + pen];
    const float* bk = vmd_rec_run(q.bucket, b, q.total_cap, q.rec3, off);
    const float inv_cx = (float)nxf * q.boxes[(size_t)VMD_BOX_STRIDE * b + 3];
    for (int c = tid; c < nxf; c += 256) s_cnt[c] = 0u;
    __syncthreads();
    for (uint32_t k = tid; k < n; k += 256) atomicAdd(&s_cnt[vmd_rec_get_cell(bk, q.rec3, k, inv_cx, nxf)], 1u);
    __syncthreads();
    // exclusive scan over the fine cells of the pencil: the counters become cursors
    // (a per-wave scan through LDS with one block barrier measured 7 % slower for this kernel than the plain block scan: profiles/r02y)
    uint32_t* cs = q.cell_start + (size_t)b * (q.ncell + 1) + (size_t)pen * nxf;
    vmd_stretch_scan<256>(s_part, nxf, tid, [&](int c) { return s_cnt[c]; }, [&](int c, uint32_t first) { s_cnt[c] = first; cs[c] = start + first; });
    if (pen == q.npen - 1 && tid == 255) q.cell_start[(size_t)b * (q.ncell + 1) + q.ncell] = start + n;
    __syncthreads();
    float* sx = s_xyz; float* sy = s_xyz + q.cap_max; float* sz = s_xyz + 2 * (size_t)q.cap_max;
    for (uint32_t k = tid; k < n; k += 256) {
        float x, y, z;
        const uint32_t c = vmd_rec_get(bk, q.rec3, k, inv_cx, nxf, x, y, z);
        const uint32_t pos = atomicAdd(&s_cnt[c], 1u);
        sx[pos] = x; sy[pos] = y; sz[pos] = z;
    }
    __syncthreads();
    float* srt = q.sorted + (size_t)b * 3 * q.nsel_pad + start;
    for (uint32_t k = tid; k < n; k += 256) {
        srt[k] = sx[k];
        srt[q.nsel_pad + k] = sy[k];
        srt[2 * (size_t)q.nsel_pad + k] = sz[k];
    }
}

// bounding box of all atoms of every frame (open axes: the pencil grid spans the box of the batch): out[b] = {min xyz, max xyz}
__global__ __launch_bounds__(1024) void k_bbox(const float* __restrict__ xyz, size_t frame_stride, size_t row_stride, int natoms,
                                               float* __restrict__ out) {
    __shared__ float s_lo[3][16], s_hi[3][16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* fx = xyz + (size_t)b * frame_stride;
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    for (int a = tid; a < natoms; a += 1024)
#pragma unroll
        for (int k = 0; k < 3; ++k) { const float v = fx[k * row_stride + a]; lo[k] = fminf(lo[k], v); hi[k] = fmaxf(hi[k], v); }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = vmd_wave_min(lo[k]); hi[k] = vmd_wave_max(hi[k]);
        if ((tid & 63) == 0) { s_lo[k][tid >> 6] = lo[k]; s_hi[k][tid >> 6] = hi[k]; }
    }
    __syncthreads();
    if (tid < 3) {
        float l = s_lo[tid][0], h = s_hi[tid][0];
        for (int w = 1; w < 16; ++w) { l = fminf(l, s_lo[tid][w]); h = fmaxf(h, s_hi[tid][w]); }
        out[6 * b + tid] = l; out[6 * b + 3 + tid] = h;
    }
}

// ------------------------------------------------------------------------------------------------ K2: RDF, pencil grid

struct vmd_pair_params_t {
    const float* __restrict__ sref; const uint32_t* __restrict__ cs_ref; int nref_pad;
    const float* __restrict__ stgt; const uint32_t* __restrict__ cs_tgt; int ntgt_pad;
    const float* __restrict__ boxes; int B;
    vmd_grid_t grid;
    vmd_binning_t bin;
    float r2_up;        // conservative candidate filter (> rmax^2)
    float rpad;         // conservative range padding (> rmax)
    uint64_t* partial;  // [gridDim.x][nbins]: one row per block, written once at the end
    unsigned long long* counts;  // the accumulators: target of the (rare) overflow flush
    unsigned* work_counter;  // [8 * VMD_COUNTER_STRIDE], zeroed before launch: one dynamic work queue per XCD (frames f = q mod 8)
    int nsub;                // work items per pencil (i-chunks are dealt round-robin to the items)
    uint32_t pbc;            // bits 0..2: periodic axes (an open axis spans the batch's bounding box: boxes slots 6..8 = origin)
    const uint32_t* skip;    // device flag or NULL: non-zero = the sorted copies are incomplete (a bucket of the cell build overflowed), do nothing
    int ry, rz;              // neighbour reach in pencils per axis: 1 (cross-section >= rmax), 2 = split pencils (cross-section >= rmax/2)
    int nsplit;              // > 1 (small launches): a chunk's neighbour pencils are dealt to nsplit work items instead of one - a lone
                             // item is a dependent chain of cold scalar loads (170 us for a one-frame launch, profiles/r03aq)
    int shift_axes;          // variant 0: an image segment with ONE live shift axis takes the loop that subtracts that shift alone (0: the general loop, A/B)
    int pop;                 // host side only: variant 0 is launched with the folded pop (instantiation POP = 2); 0 unless r_min == 0 and the fast path is usable at all
    unsigned long long* cols_total;   // device counter or NULL: candidate columns of every launch since the host last reset it (one atomic per
                                      // wave at kernel end): bench.py's "candidate lanes per counted hit" is measured, not modelled
};
#define VMD_COUNTER_STRIDE 32    // one 128-byte line per queue counter

// per-wave state of the hit machinery.  POP is part of the TYPE (the helpers below deduce it): a run-time choice between the pops - three
// inlined at every drain site, +6 KB of code, 72 instead of 68 VGPRs - cost the kernel 8 % (profiles/r06q_pop_compile_time_ab.txt).
// 0 = vmd_pop_hot, 1 = vmd_pop_hot0 (folded delta) with a plain ds_read_b32, 2 = vmd_pop_hot0 reading the stack with ds_read_addtid_b32
template <int POP>
struct vmd_wave_acc_tt {
    static constexpr int pop = POP;
    unsigned* hist;       // LDS, nbins
    float* queue;         // LDS, VMD_QUEUE_CAP floats: the wave's hit stack
    unsigned qbase;       // LDS byte address of queue[0] (0 in the emulator build, where qtop is a plain offset)
    unsigned qlim;        // qbase + 4 * VMD_WAVE: the stack holds a full wave of hits when qtop reaches it
    unsigned hbase;       // LDS byte address of hist[0] (product build only)
    unsigned qtop;        // wave-uniform: LDS byte address of the top of the stack
    float fast_c;         // bn.fast_c held in a VGPR
    float fast_k, fast_far;   // bn.fast_k / bn.fast_far in VGPRs (an SGPR operand halves the issue rate of v_fma_f32)
    float fast_c2;            // bn.fast_c2 in a VGPR (vmd_pop_hot0)
    float* slow;          // LDS, 64 floats behind the stack: hits whose fast binning was not provably exact, waiting for
    unsigned nslow;       // (wave-uniform count) a full wave of them to go through the exact path together
    unsigned ncols;       // wave-uniform: candidate columns (<= 64 hits each) since the last flush
};

// Bin `d2` of every `active` lane into the LDS histogram.  Must be called by all lanes of the wave.
// Result is exactly vmd_bin_of(d2) (SPEC S4): the 1-ulp hardware sqrt is only used where it provably cannot change the
// bin or the open-interval test; the (rare) uncertain lanes re-do the computation with the correctly rounded sqrtf.
template <unsigned INC>
__device__ __forceinline__ void vmd_bin_add(const vmd_binning_t& bn, unsigned* hist, float d2, bool active) {
    const float t = fmaf(__builtin_amdgcn_sqrtf(d2), bn.fast_k, bn.fast_c);
    int bin = (int)t;                                   // truncation: floor for the t > 0 that can be "sure"
    const float fr = t - truncf(t);
    // sure <=> t is inside bin `bin` with margin delta on both sides and the bin exists (negative t wraps to a huge unsigned)
    const bool sure = fabsf(fr - 0.5f) < bn.fast_half && (unsigned)bin < (unsigned)bn.nbins;
    bool add = active && sure;
    if (VMD_BALLOT(active && !sure)) {
        if (active && !sure) {
            bin = vmd_bin_of(bn, d2);
            add = bin >= 0;
        }
    }
    if (add) atomicAdd(&hist[bin], INC);
}

// The exact path of vmd_bin_add costs ~25 VALU instructions and used to run for 1-2 lanes at a time in every fifth pop.
// The drain therefore parks uncertain hits on a second, 64-entry LDS stack and sends them through vmd_bin_of a full wave at
// a time.  Both functions must be called by all lanes of the wave.
// (Round 6: an out-of-line version - one copy behind a three-register call instead of one per drain site, 24 -> 17 KB of code - measured
// 0.7 % SLOWER on c3, profiles/r06s_pop_ab.txt; the copies stay.)
template <unsigned INC, class W>
__device__ __forceinline__ void vmd_slow_flush(const vmd_binning_t& bn, W& w, int lane) {
    __builtin_amdgcn_wave_barrier();
    const float v = w.slow[lane];
    __builtin_amdgcn_wave_barrier();
    if ((unsigned)lane < w.nslow) {
        const int bin = vmd_bin_of(bn, v);
        if (bin >= 0) atomicAdd(&w.hist[bin], INC);
    }
    w.nslow = 0;
}
// parks the lanes of mask `m` (hits whose fast binning was not provably exact) on the slow stack
template <unsigned INC, class W>
__device__ __forceinline__ void vmd_slow_park(const vmd_binning_t& bn, W& w, float d2, unsigned long long m, bool unsure, int lane) {
    const unsigned cnt = (unsigned)__popcll(m);
    if (w.nslow + cnt > VMD_WAVE) vmd_slow_flush<INC>(bn, w, lane);
    const unsigned pre = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    if (unsure) w.slow[w.nslow + pre] = d2;
    w.nslow += cnt;
}
template <unsigned INC, class W>
__device__ __forceinline__ void vmd_bin_add_deferred(const vmd_binning_t& bn, W& w, float d2, bool active, int lane) {
    const float t = fmaf(__builtin_amdgcn_sqrtf(d2), bn.fast_k, w.fast_c);
    const int bin = vmd_floor_to_int(t);                // floor: a negative t (d < rmin) can never pass the range test below
    const float fr = vmd_fract(t);                      // t - floor(t), exact
    const bool sure = fabsf(fr - 0.5f) < bn.fast_half && (unsigned)bin < (unsigned)bn.nbins;
    if (active && sure) atomicAdd(&w.hist[bin], INC);
    const bool unsure = active && !sure;
    const unsigned long long m = VMD_BALLOT(unsure);
    if (m) vmd_slow_park<INC>(bn, w, d2, m, unsure, lane);
}
// r_min = 0, delta folded into the constant (vmd_binning_t::fast_c2 / fast_2d): t2 = t' + delta.  sure <=> fract(t2) > 2 delta, i.e. t' lies
// in (n + delta, n + 1 - delta) with n = floor(t2): the spec's scaled distance, at most delta / 2 away from t', is strictly inside bin n - the
// argument of vmd_bin_add, one rounding (the fma's) as there.  No range test: t2 >= delta > 0, and a "sure" t2 >= nbins is a distance beyond
// r_max that the padded cutoff let through (t2 < nbins * sqrt(1.0001) + delta < nbins + 1): it lands in the spare bin nbins, which nobody reads.
template <unsigned INC, class W>
__device__ __forceinline__ void vmd_bin_add_deferred0(const vmd_binning_t& bn, W& w, float d2, bool active, int lane) {
    const float t2 = fmaf(__builtin_amdgcn_sqrtf(d2), w.fast_k, w.fast_c2);
    const int bin = vmd_floor_to_int(t2);
    const bool sure = vmd_fract(t2) > bn.fast_2d;
    if (active && sure) atomicAdd(&w.hist[bin], INC);
    const bool unsure = active && !sure;
    const unsigned long long m = VMD_BALLOT(unsure);
    if (m) vmd_slow_park<INC>(bn, w, d2, m, unsure, lane);
}
#ifndef VMD_NO_INLINE_ASM
// vmd_pop_hot for r_min = 0 (every rdf() VIAMD's scripts write): 7 VALU instructions instead of 9 - v_add_f32 -0.5 and the |t| compare become
// one compare against 2 delta, the bin range compare goes (spare bin).  (k stays an SGPR operand of the fma: a VGPR would issue faster, and
// be the 73rd of a kernel that needs 72 for its seventh wave per SIMD.)
// ADDTID: the stack is read with ds_read_addtid_b32 (address = M0 + 4 * lane): the address add goes too, 6 VALU.
template <unsigned INC, bool ADDTID, class W>
__device__ __forceinline__ unsigned long long vmd_pop_hot0(const vmd_binning_t& bn, W& w, unsigned lane4, unsigned inc, float& d2) {
    unsigned long long m;
    float t;
    int b;
    if (ADDTID) {
        asm volatile(
            "s_mov_b32 m0, %[q]\n\t"
            "s_nop 0\n\t"                                   // SALU write of M0 -> LDS add-TID instruction: one wait state
            "ds_read_addtid_b32 %[d2]\n\t"
            "s_waitcnt lgkmcnt(0)\n\t"
            "v_sqrt_f32 %[t], %[d2]\n\t"
            "s_nop 0\n\t"
            "v_fma_f32 %[t], %[k], %[t], %[c]\n\t"
            "v_cvt_flr_i32_f32 %[b], %[t]\n\t"
            "v_fract_f32 %[t], %[t]\n\t"
            "v_cmp_lt_f32 vcc, %[dd], %[t]\n\t"
            "v_lshl_add_u32 %[b], %[b], 2, %[hb]\n\t"
            "s_mov_b64 exec, vcc\n\t"
            "ds_add_u32 %[b], %[inc]\n\t"
            "s_mov_b64 exec, -1\n\t"
            "s_not_b64 %[m], vcc\n\t"
            : [m] "=&s"(m), [t] "=&v"(t), [b] "=&v"(b), [d2] "=&v"(d2)
            : [q] "s"(w.qtop), [k] "s"(bn.fast_k), [c] "v"(w.fast_c2), [dd] "s"(bn.fast_2d), [hb] "s"(w.hbase), [inc] "v"(inc)
            : "vcc", "scc", "m0", "memory");
    } else {
        asm volatile(
            "v_add_u32 %[b], %[q], %[l4]\n\t"
            "ds_read_b32 %[d2], %[b]\n\t"
            "s_waitcnt lgkmcnt(0)\n\t"
            "v_sqrt_f32 %[t], %[d2]\n\t"
            "s_nop 0\n\t"
            "v_fma_f32 %[t], %[k], %[t], %[c]\n\t"
            "v_cvt_flr_i32_f32 %[b], %[t]\n\t"
            "v_fract_f32 %[t], %[t]\n\t"
            "v_cmp_lt_f32 vcc, %[dd], %[t]\n\t"
            "v_lshl_add_u32 %[b], %[b], 2, %[hb]\n\t"
            "s_mov_b64 exec, vcc\n\t"
            "ds_add_u32 %[b], %[inc]\n\t"
            "s_mov_b64 exec, -1\n\t"
            "s_not_b64 %[m], vcc\n\t"
            : [m] "=&s"(m), [t] "=&v"(t), [b] "=&v"(b), [d2] "=&v"(d2)
            : [q] "s"(w.qtop), [l4] "v"(lane4), [k] "s"(bn.fast_k), [c] "v"(w.fast_c2), [dd] "s"(bn.fast_2d), [hb] "s"(w.hbase), [inc] "v"(inc)
            : "vcc", "scc", "memory");
    }
    return m;
}
// The pop of the hot loop, hand-scheduled: read one full wave of hits from the top of the stack (w.qtop already lowered),
// fast-bin them (same arithmetic as vmd_bin_add_deferred) and ds_add under EXEC = sure mask; returns the mask of the lanes
// that must take the exact path.  9 VALU instructions; hipcc needs 14 for the same C++ (two address adds, a v_mov for the
// second uniform operand of the fma, trunc + sub instead of fract, and a v_cndmask + v_cmp round trip for the ballot).
// Requires EXEC = all lanes.
template <unsigned INC, class W>
__device__ __forceinline__ unsigned long long vmd_pop_hot(const vmd_binning_t& bn, W& w, unsigned lane4, unsigned inc, float& d2) {
    unsigned long long m;
    float t;
    int b;
    asm volatile(
        "v_add_u32 %[b], %[q], %[l4]\n\t"
        "ds_read_b32 %[d2], %[b]\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_sqrt_f32 %[t], %[d2]\n\t"
        "s_nop 0\n\t"
        "v_fma_f32 %[t], %[k], %[t], %[c]\n\t"
        "v_cvt_flr_i32_f32 %[b], %[t]\n\t"
        "v_fract_f32 %[t], %[t]\n\t"
        "v_add_f32 %[t], -0.5, %[t]\n\t"
        "v_cmp_lt_f32 %[m], |%[t]|, %[half]\n\t"
        "v_cmp_gt_u32 vcc, %[nb], %[b]\n\t"
        "s_and_b64 vcc, vcc, %[m]\n\t"
        "v_lshl_add_u32 %[b], %[b], 2, %[hb]\n\t"
        "s_mov_b64 exec, vcc\n\t"
        "ds_add_u32 %[b], %[inc]\n\t"
        "s_mov_b64 exec, -1\n\t"
        "s_not_b64 %[m], vcc\n\t"
        : [m] "=&s"(m), [t] "=&v"(t), [b] "=&v"(b), [d2] "=&v"(d2)
        : [q] "s"(w.qtop), [l4] "v"(lane4), [k] "s"(bn.fast_k), [c] "v"(w.fast_c), [half] "s"(bn.fast_half),
          [nb] "s"(bn.nbins), [hb] "s"(w.hbase), [inc] "v"(inc)
        : "vcc", "scc", "memory");
    return m;
}
#endif

// variant 2: the same with the "certainly outside" test in front of the parking (a pair entry's partner is usually no hit)
template <unsigned INC, class W>
__device__ __forceinline__ void vmd_bin_add_deferred_far(const vmd_binning_t& bn, W& w, float d2, bool active, int lane) {
    const float t = fmaf(__builtin_amdgcn_sqrtf(d2), bn.fast_k, w.fast_c);
    const int bin = vmd_floor_to_int(t);
    const float fr = vmd_fract(t);
    const bool sure = fabsf(fr - 0.5f) < bn.fast_half && (unsigned)bin < (unsigned)bn.nbins;
    if (active && sure) atomicAdd(&w.hist[bin], INC);
    const bool unsure = active && !sure && t < bn.fast_far;
    const unsigned long long m = VMD_BALLOT(unsure);
    if (m) vmd_slow_park<INC>(bn, w, d2, m, unsure, lane);
}
#ifndef VMD_NO_INLINE_ASM
// variant 2 pop: 64 pair entries = 128 values, two interleaved binning chains; returns the two park masks.  19 VALU.
template <unsigned INC, class W>
__device__ __forceinline__ void vmd_pop_hot2(const vmd_binning_t& bn, W& w, unsigned lane8 /* 4 * lane: entries are slots of 4 bytes */, unsigned inc, float& a, float& b,
                                             unsigned long long& ma, unsigned long long& mb) {
    unsigned long long sa;
    float ta, tb;
    int ba, bb;
    asm volatile(
        "v_add_u32 %[ba], %[q], %[l8]\n\t"
        "ds_read_b32 %[a], %[ba]\n\t"
        "ds_read_b32 %[b], %[ba] offset:512\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_sqrt_f32 %[ta], %[a]\n\t"
        "v_sqrt_f32 %[tb], %[b]\n\t"
        "s_nop 0\n\t"
        "v_fma_f32 %[ta], %[k], %[ta], %[c]\n\t"
        "v_fma_f32 %[tb], %[k], %[tb], %[c]\n\t"
        "v_cvt_flr_i32_f32 %[ba], %[ta]\n\t"
        "v_cvt_flr_i32_f32 %[bb], %[tb]\n\t"
        "v_cmp_gt_f32 %[ma], %[far], %[ta]\n\t"
        "v_cmp_gt_f32 %[mb], %[far], %[tb]\n\t"
        "v_fract_f32 %[ta], %[ta]\n\t"
        "v_fract_f32 %[tb], %[tb]\n\t"
        "v_add_f32 %[ta], -0.5, %[ta]\n\t"
        "v_add_f32 %[tb], -0.5, %[tb]\n\t"
        "v_cmp_lt_f32 %[sa], |%[ta]|, %[half]\n\t"
        "v_cmp_gt_u32 vcc, %[nb], %[ba]\n\t"
        "s_and_b64 vcc, vcc, %[sa]\n\t"
        "s_andn2_b64 %[ma], %[ma], vcc\n\t"
        "v_lshl_add_u32 %[ba], %[ba], 2, %[hb]\n\t"
        "s_mov_b64 exec, vcc\n\t"
        "ds_add_u32 %[ba], %[inc]\n\t"
        "s_mov_b64 exec, -1\n\t"
        "v_cmp_lt_f32 %[sa], |%[tb]|, %[half]\n\t"
        "v_cmp_gt_u32 vcc, %[nb], %[bb]\n\t"
        "s_and_b64 vcc, vcc, %[sa]\n\t"
        "s_andn2_b64 %[mb], %[mb], vcc\n\t"
        "v_lshl_add_u32 %[bb], %[bb], 2, %[hb]\n\t"
        "s_mov_b64 exec, vcc\n\t"
        "ds_add_u32 %[bb], %[inc]\n\t"
        "s_mov_b64 exec, -1\n\t"
        : [ma] "=&s"(ma), [mb] "=&s"(mb), [sa] "=&s"(sa), [ta] "=&v"(ta), [tb] "=&v"(tb), [ba] "=&v"(ba), [bb] "=&v"(bb), [a] "=&v"(a), [b] "=&v"(b)
        : [q] "s"(w.qtop), [l8] "v"(lane8), [k] "v"(w.fast_k), [c] "v"(w.fast_c), [far] "v"(w.fast_far), [half] "s"(bn.fast_half),
          [nb] "s"(bn.nbins), [hb] "s"(w.hbase), [inc] "v"(inc)
        : "vcc", "scc", "memory");
}
#endif

// variant 2: TWO candidate columns share one compaction.  A lane whose smaller d2 of the pair is a candidate pushes both
// values as one entry: slot s of the stack holds the first value at queue[s] and the second at queue[VMD_PAIR_B + s] (two
// conflict-free 4-byte accesses per lane instead of one 8-byte access with a 2-way bank conflict); the pop bins both and drops the
// partner that is no hit with one compare.  Per pair of columns: v_min + v_cmp + 2 v_mbcnt + v_lshl_add + one ds_write_b64 instead of
// 2 x (v_cmp + 2 v_mbcnt + v_lshl_add + ds_write_b32): the integer ops of the prefix issue at 4 cycles per wave whatever their
// operands are (profiles/r02_valu_calibration.txt), so halving them is what counts; the pop handles ~1.85 values per hit.
template <class W>
__device__ __forceinline__ void vmd_push2(W& w, bool hit, float a, float b) {
    const unsigned long long mask = VMD_BALLOT(hit);
    if (mask) {
        const unsigned pre = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        if (hit) {
            float* e = (float*)((char*)w.queue + ((w.qtop - w.qbase) + 4u * pre));
            e[0] = a; e[VMD_PAIR_B] = b;
        }
        w.qtop += 4u * (unsigned)__popcll(mask);
    }
}

// VARIANT 0: compact the hits of one candidate column onto the wave's LDS stack (order is irrelevant for a
// histogram, so LIFO: no head pointer, no wrap-around); vmd_drain_full pops full waves of 64 so that
// sqrt + binning + ds_add always run with every lane busy.
// VARIANT 1: bin the hits in place under the divergent mask (same arithmetic; A/B baseline and cross-check).
template <int VARIANT, unsigned INC, class W>
__device__ __forceinline__ void vmd_push(const vmd_binning_t& bn, W& w, bool hit, float d2) {
    if (VARIANT == 1) {
        vmd_bin_add<INC>(bn, w.hist, d2, hit);
        return;
    }
    if (VARIANT == 2) { vmd_push2(w, hit, d2, VMD_JUNK); return; }
    const unsigned long long mask = VMD_BALLOT(hit);
    if (mask) {
        const unsigned pre = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        if (hit) *(float*)((char*)w.queue + ((w.qtop - w.qbase) + 4u * pre)) = d2;
        w.qtop += 4u * (unsigned)__popcll(mask);
    }
}

template <int VARIANT, unsigned INC, class W>
__device__ __forceinline__ void vmd_drain_full(const vmd_binning_t& bn, W& w, int lane) {
    if (VARIANT == 1) return;
    if (VARIANT == 2) {
        while (w.qtop - w.qbase >= 4u * VMD_WAVE) {
            w.qtop -= 4u * VMD_WAVE;
            float a, b;
#ifndef VMD_NO_INLINE_ASM
            unsigned long long ma, mb;
            vmd_pop_hot2<INC>(bn, w, 4u * (unsigned)lane, INC, a, b, ma, mb);
            if (ma) vmd_slow_park<INC>(bn, w, a, ma, (ma >> lane) & 1ull, lane);
            if (mb) vmd_slow_park<INC>(bn, w, b, mb, (mb >> lane) & 1ull, lane);
#else
            __builtin_amdgcn_wave_barrier();
            const float* e = (const float*)((const char*)w.queue + ((w.qtop - w.qbase) + 4u * (unsigned)lane));
            a = e[0]; b = e[VMD_PAIR_B];
            __builtin_amdgcn_wave_barrier();
            vmd_bin_add_deferred_far<INC>(bn, w, a, true, lane);
            vmd_bin_add_deferred_far<INC>(bn, w, b, true, lane);
#endif
        }
        return;
    }
    while (w.qtop >= w.qlim) {      // (against a kept limit: s_cmp + branch; `qtop - qbase >= 256` is one SALU instruction more per group of four
                                    // columns, and this loop feels every one of them - c3 -1.2 %, profiles/r06v_salu_ab.txt)
        w.qtop -= 4u * VMD_WAVE;
#ifndef VMD_NO_INLINE_ASM
        float v;
        const unsigned long long m = W::pop == 2 ? vmd_pop_hot0<INC, true>(bn, w, 4u * (unsigned)lane, INC, v)
                                   : W::pop == 1 ? vmd_pop_hot0<INC, false>(bn, w, 4u * (unsigned)lane, INC, v)
                                                 : vmd_pop_hot<INC>(bn, w, 4u * (unsigned)lane, INC, v);
        if (m) vmd_slow_park<INC>(bn, w, v, m, (m >> lane) & 1ull, lane);
#else
        __builtin_amdgcn_wave_barrier();
        const float v = *(const float*)((const char*)w.queue + ((w.qtop - w.qbase) + 4u * (unsigned)lane));
        __builtin_amdgcn_wave_barrier();
        if (W::pop) vmd_bin_add_deferred0<INC>(bn, w, v, true, lane);
        else vmd_bin_add_deferred<INC>(bn, w, v, true, lane);
#endif
    }
}

template <int VARIANT, unsigned INC, class W>
__device__ __forceinline__ void vmd_drain(const vmd_binning_t& bn, W& w, int lane) {
    if (VARIANT == 1) return;
    vmd_drain_full<VARIANT, INC>(bn, w, lane);
    if (VARIANT == 2) {
        const unsigned rem = (w.qtop - w.qbase) / 4u;
        __builtin_amdgcn_wave_barrier();
        const float a = w.queue[lane], b = w.queue[VMD_PAIR_B + lane];
        __builtin_amdgcn_wave_barrier();
        w.qtop = w.qbase;
        vmd_bin_add_deferred_far<INC>(bn, w, a, (unsigned)lane < rem, lane);
        vmd_bin_add_deferred_far<INC>(bn, w, b, (unsigned)lane < rem, lane);
        vmd_slow_flush<INC>(bn, w, lane);
        return;
    }
    const unsigned rem = (w.qtop - w.qbase) / 4u;
    __builtin_amdgcn_wave_barrier();
    const float v = w.queue[lane];
    __builtin_amdgcn_wave_barrier();
    w.qtop = w.qbase;
    if (W::pop) vmd_bin_add_deferred0<INC>(bn, w, v, (unsigned)lane < rem, lane);
    else vmd_bin_add_deferred<INC>(bn, w, v, (unsigned)lane < rem, lane);
    vmd_slow_flush<INC>(bn, w, lane);
}

// The push of the hot loop, hand-scheduled (hipcc spends 8 SALU + 5 VALU per column on the same thing): compare, and if
// any lane hit, prefix the hit lanes (v_mbcnt), store their d2 on the LDS stack under EXEC = hit mask, advance the stack.
// Requires EXEC = all 64 lanes on entry (true in the segment loops: padding lanes carry far-away coordinates instead of
// being masked off).  The SIMT emulator build (tests/emu) has no inline asm and takes the plain C++ vmd_push instead.
#ifndef VMD_NO_INLINE_ASM
#define VMD_PUSH_NOP "s_nop 0\n\t"      // (dropping it changes neither results nor speed on gfx950, profiles/r06v_salu_ab.txt; the VOP3P -> VALU wait state stays explicit)
#define VMD_LDS_ADDRESS(p) ((unsigned)(size_t)(__attribute__((address_space(3))) void*)(p))
template <class W>
__device__ __forceinline__ void vmd_push_hot(W& w, float d2, float r2) {
    unsigned t, n;
    // s_nop: d2 usually comes straight out of a v_pk_fma_f32; the hazard recogniser cannot see into this block and the
    // VOP3P result needs one wait state before a dependent VALU read on gfx940-class parts
    asm volatile(
        "s_nop 0\n\t"
        "v_cmp_gt_f32 vcc, %[r2], %[d2]\n\t"
        "s_cbranch_vccz .Lvmd_nohit%=\n\t"
        "v_mbcnt_lo_u32_b32 %[t], vcc_lo, 0\n\t"
        "v_mbcnt_hi_u32_b32 %[t], vcc_hi, %[t]\n\t"
        "v_lshl_add_u32 %[t], %[t], 2, %[q]\n\t"
        "s_mov_b64 exec, vcc\n\t"
        "ds_write_b32 %[t], %[d2]\n\t"
        "s_mov_b64 exec, -1\n\t"
        "s_bcnt1_i32_b64 %[n], vcc\n\t"
        "s_lshl2_add_u32 %[q], %[n], %[q]\n"
        ".Lvmd_nohit%=:"
        : [q] "+s"(w.qtop), [t] "=&v"(t), [n] "=&s"(n)
        : [d2] "v"(d2), [r2] "s"(r2)
        : "vcc", "scc", "memory");
}
// same with the own-pencil condition j > i folded in (j wave-uniform, i per lane)
template <class W>
__device__ __forceinline__ void vmd_push_hot_masked(W& w, float d2, float r2, unsigned j, unsigned i) {
    unsigned t, n;
    unsigned long long m;
    asm volatile(
        "s_nop 0\n\t"
        "v_cmp_gt_f32 vcc, %[r2], %[d2]\n\t"
        "v_cmp_gt_u32 %[m], %[j], %[i]\n\t"
        "s_and_b64 vcc, vcc, %[m]\n\t"
        "s_cbranch_scc0 .Lvmd_nohitm%=\n\t"
        "v_mbcnt_lo_u32_b32 %[t], vcc_lo, 0\n\t"
        "v_mbcnt_hi_u32_b32 %[t], vcc_hi, %[t]\n\t"
        "v_lshl_add_u32 %[t], %[t], 2, %[q]\n\t"
        "s_mov_b64 exec, vcc\n\t"
        "ds_write_b32 %[t], %[d2]\n\t"
        "s_mov_b64 exec, -1\n\t"
        "s_bcnt1_i32_b64 %[n], vcc\n\t"
        "s_lshl2_add_u32 %[q], %[n], %[q]\n"
        ".Lvmd_nohitm%=:"
        : [q] "+s"(w.qtop), [t] "=&v"(t), [n] "=&s"(n), [m] "=&s"(m)
        : [d2] "v"(d2), [r2] "s"(r2), [j] "s"(j), [i] "v"(i)
        : "vcc", "scc", "memory");
}
// Four columns per asm block: consecutive blocks each drew a hazard nop from the compiler (which cannot see inside) on top
// of their own, and pinned the order of the packed chains around them; one block per s_load group needs a single wait
// state and lets hipcc interleave the two packed d2 chains in front of it.
template <class W>
__device__ __forceinline__ void vmd_push_hot4(W& w, float d0, float d1, float d2, float d3, float r2) {
    unsigned t, n;
    asm volatile(
        VMD_PUSH_NOP
        "v_cmp_gt_f32 vcc, %[r2], %[d0]\n\t"
        "s_cbranch_vccz .Lvmd_p4_0_%=\n\t"
        "v_mbcnt_lo_u32_b32 %[t], vcc_lo, 0\n\t"
        "v_mbcnt_hi_u32_b32 %[t], vcc_hi, %[t]\n\t"
        "v_lshl_add_u32 %[t], %[t], 2, %[q]\n\t"
        "s_mov_b64 exec, vcc\n\t"
        "ds_write_b32 %[t], %[d0]\n\t"
        "s_mov_b64 exec, -1\n\t"
        "s_bcnt1_i32_b64 %[n], vcc\n\t"
        "s_lshl2_add_u32 %[q], %[n], %[q]\n"
        ".Lvmd_p4_0_%=:\n\t"
        "v_cmp_gt_f32 vcc, %[r2], %[d1]\n\t"
        "s_cbranch_vccz .Lvmd_p4_1_%=\n\t"
        "v_mbcnt_lo_u32_b32 %[t], vcc_lo, 0\n\t"
        "v_mbcnt_hi_u32_b32 %[t], vcc_hi, %[t]\n\t"
        "v_lshl_add_u32 %[t], %[t], 2, %[q]\n\t"
        "s_mov_b64 exec, vcc\n\t"
        "ds_write_b32 %[t], %[d1]\n\t"
        "s_mov_b64 exec, -1\n\t"
        "s_bcnt1_i32_b64 %[n], vcc\n\t"
        "s_lshl2_add_u32 %[q], %[n], %[q]\n"
        ".Lvmd_p4_1_%=:\n\t"
        "v_cmp_gt_f32 vcc, %[r2], %[d2]\n\t"
        "s_cbranch_vccz .Lvmd_p4_2_%=\n\t"
        "v_mbcnt_lo_u32_b32 %[t], vcc_lo, 0\n\t"
        "v_mbcnt_hi_u32_b32 %[t], vcc_hi, %[t]\n\t"
        "v_lshl_add_u32 %[t], %[t], 2, %[q]\n\t"
        "s_mov_b64 exec, vcc\n\t"
        "ds_write_b32 %[t], %[d2]\n\t"
        "s_mov_b64 exec, -1\n\t"
        "s_bcnt1_i32_b64 %[n], vcc\n\t"
        "s_lshl2_add_u32 %[q], %[n], %[q]\n"
        ".Lvmd_p4_2_%=:\n\t"
        "v_cmp_gt_f32 vcc, %[r2], %[d3]\n\t"
        "s_cbranch_vccz .Lvmd_p4_3_%=\n\t"
        "v_mbcnt_lo_u32_b32 %[t], vcc_lo, 0\n\t"
        "v_mbcnt_hi_u32_b32 %[t], vcc_hi, %[t]\n\t"
        "v_lshl_add_u32 %[t], %[t], 2, %[q]\n\t"
        "s_mov_b64 exec, vcc\n\t"
        "ds_write_b32 %[t], %[d3]\n\t"
        "s_mov_b64 exec, -1\n\t"
        "s_bcnt1_i32_b64 %[n], vcc\n\t"
        "s_lshl2_add_u32 %[q], %[n], %[q]\n"
        ".Lvmd_p4_3_%=:\n\t"
        : [q] "+s"(w.qtop), [t] "=&v"(t), [n] "=&s"(n)
        : [d0] "v"(d0), [d1] "v"(d1), [d2] "v"(d2), [d3] "v"(d3), [r2] "s"(r2)
        : "vcc", "scc", "memory");
}
// own pencil: column j counts only j > i.  Lane L holds atom cbeg + L, so column j passes exactly the lanes 0 .. j - cbeg - 1: a wave-uniform
// mask, made on the scalar unit (until now a v_cmp_gt_i32 per column against i, i - 1, i - 2, i - 3 in four VGPRs).  nm is the COMPLEMENT of
// the current column's mask, ~0 << (j - cbeg), and moves one lane up behind every column: s_andn2 takes it out of the hits (SCC = any left,
// as the s_and before it), s_lshl_b64 - which writes SCC too - waits behind the branch.  A width of 64 or more (only columns past the
// segment: at -VMD_FAR, never a hit) shifts nm out to 0 = all lanes; no width wraps around into an empty or partial mask.
template <class W>
__device__ __forceinline__ void vmd_push_hot4_masked(W& w, float d0, float d1, float d2, float d3, float r2, unsigned long long& nm) {
    unsigned t, n;
    asm volatile(
        VMD_PUSH_NOP
        "v_cmp_gt_f32 vcc, %[r2], %[d0]\n\t"
        "s_andn2_b64 vcc, vcc, %[nm]\n\t"
        "s_cbranch_scc0 .Lvmd_p4m_0_%=\n\t"
        "v_mbcnt_lo_u32_b32 %[t], vcc_lo, 0\n\t"
        "v_mbcnt_hi_u32_b32 %[t], vcc_hi, %[t]\n\t"
        "v_lshl_add_u32 %[t], %[t], 2, %[q]\n\t"
        "s_mov_b64 exec, vcc\n\t"
        "ds_write_b32 %[t], %[d0]\n\t"
        "s_mov_b64 exec, -1\n\t"
        "s_bcnt1_i32_b64 %[n], vcc\n\t"
        "s_lshl2_add_u32 %[q], %[n], %[q]\n"
        ".Lvmd_p4m_0_%=:\n\t"
        "s_lshl_b64 %[nm], %[nm], 1\n\t"
        "v_cmp_gt_f32 vcc, %[r2], %[d1]\n\t"
        "s_andn2_b64 vcc, vcc, %[nm]\n\t"
        "s_cbranch_scc0 .Lvmd_p4m_1_%=\n\t"
        "v_mbcnt_lo_u32_b32 %[t], vcc_lo, 0\n\t"
        "v_mbcnt_hi_u32_b32 %[t], vcc_hi, %[t]\n\t"
        "v_lshl_add_u32 %[t], %[t], 2, %[q]\n\t"
        "s_mov_b64 exec, vcc\n\t"
        "ds_write_b32 %[t], %[d1]\n\t"
        "s_mov_b64 exec, -1\n\t"
        "s_bcnt1_i32_b64 %[n], vcc\n\t"
        "s_lshl2_add_u32 %[q], %[n], %[q]\n"
        ".Lvmd_p4m_1_%=:\n\t"
        "s_lshl_b64 %[nm], %[nm], 1\n\t"
        "v_cmp_gt_f32 vcc, %[r2], %[d2]\n\t"
        "s_andn2_b64 vcc, vcc, %[nm]\n\t"
        "s_cbranch_scc0 .Lvmd_p4m_2_%=\n\t"
        "v_mbcnt_lo_u32_b32 %[t], vcc_lo, 0\n\t"
        "v_mbcnt_hi_u32_b32 %[t], vcc_hi, %[t]\n\t"
        "v_lshl_add_u32 %[t], %[t], 2, %[q]\n\t"
        "s_mov_b64 exec, vcc\n\t"
        "ds_write_b32 %[t], %[d2]\n\t"
        "s_mov_b64 exec, -1\n\t"
        "s_bcnt1_i32_b64 %[n], vcc\n\t"
        "s_lshl2_add_u32 %[q], %[n], %[q]\n"
        ".Lvmd_p4m_2_%=:\n\t"
        "s_lshl_b64 %[nm], %[nm], 1\n\t"
        "v_cmp_gt_f32 vcc, %[r2], %[d3]\n\t"
        "s_andn2_b64 vcc, vcc, %[nm]\n\t"
        "s_cbranch_scc0 .Lvmd_p4m_3_%=\n\t"
        "v_mbcnt_lo_u32_b32 %[t], vcc_lo, 0\n\t"
        "v_mbcnt_hi_u32_b32 %[t], vcc_hi, %[t]\n\t"
        "v_lshl_add_u32 %[t], %[t], 2, %[q]\n\t"
        "s_mov_b64 exec, vcc\n\t"
        "ds_write_b32 %[t], %[d3]\n\t"
        "s_mov_b64 exec, -1\n\t"
        "s_bcnt1_i32_b64 %[n], vcc\n\t"
        "s_lshl2_add_u32 %[q], %[n], %[q]\n"
        ".Lvmd_p4m_3_%=:\n\t"
        "s_lshl_b64 %[nm], %[nm], 1\n\t"
        : [q] "+s"(w.qtop), [nm] "+s"(nm), [t] "=&v"(t), [n] "=&s"(n)
        : [d0] "v"(d0), [d1] "v"(d1), [d2] "v"(d2), [d3] "v"(d3), [r2] "s"(r2)
        : "vcc", "scc", "memory");
}
// variant 2: one pair-column (two candidate columns), a / b = its two d2 values.  The stack is drained after every pair-column, so it
// never holds more than 64 + 64 entries.
template <class W>
__device__ __forceinline__ void vmd_push_hot2p(W& w, float a, float b, float r2) {
    unsigned t, n;
    float m;
    asm volatile(
        "s_nop 0\n\t"
        "v_min_f32 %[m], %[a], %[b]\n\t"
        "v_cmp_gt_f32 vcc, %[r2], %[m]\n\t"
        "s_cbranch_vccz .Lvmd_pp_%=\n\t"
        "v_mbcnt_lo_u32_b32 %[t], vcc_lo, 0\n\t"
        "v_mbcnt_hi_u32_b32 %[t], vcc_hi, %[t]\n\t"
        "v_lshl_add_u32 %[t], %[t], 2, %[q]\n\t"
        "s_mov_b64 exec, vcc\n\t"
        "ds_write_b32 %[t], %[a]\n\t"
        "ds_write_b32 %[t], %[b] offset:512\n\t"
        "s_mov_b64 exec, -1\n\t"
        "s_bcnt1_i32_b64 %[n], vcc\n\t"
        "s_lshl2_add_u32 %[q], %[n], %[q]\n"
        ".Lvmd_pp_%=:\n\t"
        : [q] "+s"(w.qtop), [t] "=&v"(t), [n] "=&s"(n), [m] "=&v"(m)
        : [a] "v"(a), [b] "v"(b), [r2] "s"(r2)
        : "vcc", "scc", "memory");
}
// own pencil: the chunk against itself.  Lane L holds atom cbeg + L; the pair-column (j, j + 1) counts for the lanes L <= j - cbeg
// only (unordered pairs once; on lane L == j - cbeg the first value is the atom's distance to itself: the caller replaces it by
// VMD_JUNK).  lm: that lane mask, wave-uniform.
template <class W>
__device__ __forceinline__ void vmd_push_hot2p_masked(W& w, float a, float b, float r2, unsigned long long lm) {
    unsigned t, n;
    float m;
    asm volatile(
        "s_nop 0\n\t"
        "v_min_f32 %[m], %[a], %[b]\n\t"
        "v_cmp_gt_f32 vcc, %[r2], %[m]\n\t"
        "s_and_b64 vcc, vcc, %[lm]\n\t"
        "s_cbranch_scc0 .Lvmd_ppm_%=\n\t"
        "v_mbcnt_lo_u32_b32 %[t], vcc_lo, 0\n\t"
        "v_mbcnt_hi_u32_b32 %[t], vcc_hi, %[t]\n\t"
        "v_lshl_add_u32 %[t], %[t], 2, %[q]\n\t"
        "s_mov_b64 exec, vcc\n\t"
        "ds_write_b32 %[t], %[a]\n\t"
        "ds_write_b32 %[t], %[b] offset:512\n\t"
        "s_mov_b64 exec, -1\n\t"
        "s_bcnt1_i32_b64 %[n], vcc\n\t"
        "s_lshl2_add_u32 %[q], %[n], %[q]\n"
        ".Lvmd_ppm_%=:\n\t"
        : [q] "+s"(w.qtop), [t] "=&v"(t), [n] "=&s"(n), [m] "=&v"(m)
        : [a] "v"(a), [b] "v"(b), [r2] "s"(r2), [lm] "s"(lm)
        : "vcc", "scc", "memory");
}
#else
#define VMD_LDS_ADDRESS(p) 0u
#endif

// one uniform j segment [ja, jb) against the wave's 64 i atoms.  MASKED: count only j > i (own pencil, same set).
// AXES (bit 0: x, 1: y, 2: z): the segment is a periodic image, displaced by (sx,sy,sz) (SPEC S3: dx = fl(fl(xi-xj) - sx)), and these are the
// axes whose shift is subtracted.  An axis may be left out when its shift is a zero: fl(d - +-0) is d, but for the sign of a zero d, and d is
// squared next - d2 has the same bits.  0: no image; 1, 2, 4: the one live axis of nearly every image of an orthorhombic cell; 7: any shift.
template <int VARIANT, unsigned INC, bool MASKED, int AXES, class W>
__device__ __forceinline__ void vmd_segment_loop(const vmd_pair_params_t& p, W& w, vmd_cf32* tx, vmd_cf32* ty, vmd_cf32* tz,
                                                 unsigned ja, unsigned jb, float sx, float sy, float sz,
                                                 float xi, float yi, float zi, unsigned i, unsigned cbeg, int lane) {
    const float r2 = p.r2_up;
    const unsigned n = jb - ja;
    // two j columns per VALU instruction: v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 are IEEE per element, so the
    // arithmetic is still SPEC S3 exactly; the j pair sits in an SGPR pair straight from s_load_dwordx4
    const vmd_f2 xi2 = {xi, xi}, yi2 = {yi, yi}, zi2 = {zi, zi};
    const vmd_f2 sx2 = {sx, sx}, sy2 = {sy, sy}, sz2 = {sz, sz};
    // own pencil, variant 0: the lanes that do NOT pass the next column (vmd_push_hot4_masked).  The masked segment starts at ja >= cbeg and
    // ends at cbeg + 64 at the latest; the groups take the columns in order, each push moves the mask on by its four
    unsigned long long nm = MASKED ? ~0ull << ((ja - cbeg) & 63u) : 0ull;
    // four columns (two packed pairs) from one s_load_dwordx4 per coordinate
    auto group = [&](const vmd_f4& xj, const vmd_f4& yj, const vmd_f4& zj, unsigned j0) {       // j0: the group's first column
        vmd_f2 d2[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const vmd_f2 xj2 = {xj[2 * h], xj[2 * h + 1]}, yj2 = {yj[2 * h], yj[2 * h + 1]}, zj2 = {zj[2 * h], zj[2 * h + 1]};
            vmd_f2 dx = xi2 - xj2, dy = yi2 - yj2, dz = zi2 - zj2;
            if (AXES & 1) dx = dx - sx2;
            if (AXES & 2) dy = dy - sy2;
            if (AXES & 4) dz = dz - sz2;
            d2[h] = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
        }
#ifndef VMD_NO_INLINE_ASM
        if (VARIANT == 0) {
            if (MASKED) vmd_push_hot4_masked(w, d2[0][0], d2[0][1], d2[1][0], d2[1][1], r2, nm);
            else vmd_push_hot4(w, d2[0][0], d2[0][1], d2[1][0], d2[1][1], r2);
            vmd_drain_full<VARIANT, INC>(p.bin, w, lane);
            return;
        }
        if (VARIANT == 2) {
            if (MASKED) {
                // lanes 0 .. (j - cbeg) of the pair-column starting at j; the chunk starts at the atom of lane 0
                const int a = (int)j0 - __builtin_amdgcn_readfirstlane((int)i);
                const unsigned long long lm0 = a >= 63 ? ~0ull : ((2ull << a) - 1ull);
                const unsigned long long lm1 = a + 2 >= 63 ? ~0ull : ((2ull << (a + 2)) - 1ull);
                // the self pair (lane a of the first column, lane a + 2 of the third) never enters the stack
                const float s0 = lane == a ? VMD_JUNK : d2[0][0];
                const float s1 = lane == a + 2 ? VMD_JUNK : d2[1][0];
                vmd_push_hot2p_masked(w, s0, d2[0][1], r2, lm0);
                vmd_drain_full<VARIANT, INC>(p.bin, w, lane);
                vmd_push_hot2p_masked(w, s1, d2[1][1], r2, lm1);
            } else {
                vmd_push_hot2p(w, d2[0][0], d2[0][1], r2);
                vmd_drain_full<VARIANT, INC>(p.bin, w, lane);
                vmd_push_hot2p(w, d2[1][0], d2[1][1], r2);
            }
            vmd_drain_full<VARIANT, INC>(p.bin, w, lane);
            return;
        }
#endif
        if (VARIANT == 2) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float a = d2[h][0], b = d2[h][1];
                if (MASKED) { if (!(j0 + 2 * h > i)) a = VMD_JUNK; if (!(j0 + 2 * h + 1 > i)) b = VMD_JUNK; }
                vmd_push2(w, fminf(a, b) < r2, a, b);
                vmd_drain_full<VARIANT, INC>(p.bin, w, lane);
            }
            return;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float v = d2[c >> 1][c & 1];
            bool hit = v < r2;
            if (MASKED) hit = hit && (unsigned)lane < j0 + c - cbeg;      // the low j - cbeg lanes, all of them from 64 on: the twin of the scalar mask
            vmd_push<VARIANT, INC>(p.bin, w, hit, v);
        }
        vmd_drain_full<VARIANT, INC>(p.bin, w, lane);
    };
    // software pipeline: the scalar loads of the next group are issued before the current group is processed (two register
    // sets, no copies).  Loads may run up to 16 bytes past the segment: the sorted rows carry that much slack.
    // The ragged end (n mod 8 columns) goes through the same packed group, its columns beyond the segment moved out of every cutoff
    // (x = -VMD_FAR: never a hit, for valid and padding lanes alike) - until round 6 a one-column loop with the plain C++ push and a
    // drain of its own: ~1 % of the columns at twice the price (c3: 71.9 -> 71.3 ms per 1 000 frames, profiles/r06r_tail_ab.txt).
    if (n == 0) return;
    // the three rows are addressed from their starts, the segment by its byte offset 4 * ja: the row pointers are the same for every segment of
    // the item and need no copy advanced by ja (three 64-bit additions per segment, into six more scalar registers)
    unsigned off = 4u * ja;
    vmd_f4 xa = vmd_uniform_load4(tx, off), ya = vmd_uniform_load4(ty, off), za = vmd_uniform_load4(tz, off);
    // the loop counts BYTES of the j rows and runs against a kept last offset: add + compare + one backward branch per eight columns (counting
    // columns it was add, compare, two branches, a register copy and a shift; every scalar instruction of this loop shows, profiles/r06v_salu_ab.txt)
    if (n >= 8) {
        const unsigned stop = 4u * jb - 32u;
        do {
            const vmd_f4 xb = vmd_uniform_load4(tx, off + 16u), yb = vmd_uniform_load4(ty, off + 16u), zb = vmd_uniform_load4(tz, off + 16u);
            group(xa, ya, za, off >> 2);
            xa = vmd_uniform_load4(tx, off + 32u); ya = vmd_uniform_load4(ty, off + 32u); za = vmd_uniform_load4(tz, off + 32u);
            group(xb, yb, zb, (off >> 2) + 4u);
            off += 32u;
        } while (off <= stop);
    }
    unsigned j = off >> 2;
    while (j < jb) {                                  // at most twice: xa / ya / za hold columns j .. j + 3
        const unsigned r = jb - j;
        vmd_f4 xb = xa, yb = ya, zb = za;
        if (r > 4) { xb = vmd_uniform_load4(tx, 4u * j + 16u); yb = vmd_uniform_load4(ty, 4u * j + 16u); zb = vmd_uniform_load4(tz, 4u * j + 16u); }
        if (r < 4) {
            xa[3] = -VMD_FAR;
            if (r < 3) xa[2] = -VMD_FAR;
            if (r < 2) xa[1] = -VMD_FAR;
        }
        group(xa, ya, za, j);
        j += 4;
        xa = xb; ya = yb; za = zb;
    }
    vmd_drain_full<VARIANT, INC>(p.bin, w, lane);
}

// VARIANT 3 (A/B): the j atoms of a segment are first tested, 64 at a time (one per lane), against the bounding box of the wave's
// i atoms; only those within reach of the box become candidate columns.  The segment's window is the box-shaped dilation of the
// chunk (whole neighbour pencils x an x range); ~30 % of its atoms are farther than r from every point of the chunk's box (the corners
// of the diagonal pencils, the ends of the x range) and would be columns without a single hit.  Survivors are taken off the ballot
// mask four at a time (s_ff1 / s_bitset0), their coordinates come through scalar loads as before, and the same packed filter and
// push run on them; a short last group is padded with far-away columns.  Conservative by construction: the box distance is a lower
// bound of every lane's distance, compared against the padded cutoff - results are bit-identical.
// Measured (profiles/r02r_ab_variant3.txt): 31 % fewer columns, but c3 runs at 8.1k instead of 12.5k frames/s: the bit scan and the
// per-survivor addressing cost ~9 SALU instructions per column on top of the push's 5, and an SALU instruction takes the same
// 4.2-cycle issue slot of the SIMD as the slow VALU classes (profiles/r02_valu_calibration.txt) - the loop turns SALU-issue bound;
// twelve one-dword scalar requests per group instead of three 16-byte ones do the rest.  Kept as a checked option, off.
struct vmd_bbox_t { float lox, hix, loy, hiy, loz, hiz, rp2; };

// lowest set bit of a wave-uniform mask (-1 when empty) / clear bit k (k & 63) - one SALU instruction each
#ifndef VMD_NO_INLINE_ASM
__device__ __forceinline__ int vmd_sff1(unsigned long long m) { int k; asm("s_ff1_i32_b64 %0, %1" : "=s"(k) : "s"(m)); return k; }
__device__ __forceinline__ unsigned long long vmd_sbitclr(unsigned long long m, int k) { asm("s_bitset0_b64 %0, %1" : "+s"(m) : "s"(k)); return m; }
#else
__device__ __forceinline__ int vmd_sff1(unsigned long long m) { return m ? __builtin_ctzll(m) : -1; }
__device__ __forceinline__ unsigned long long vmd_sbitclr(unsigned long long m, int k) { return m & ~(1ull << (k & 63)); }
#endif
// one wave-uniform float at byte offset `off` (s_load_dword sdst, sbase, soffset)
__device__ __forceinline__ float vmd_uniform_load1(vmd_cf32* base, unsigned off) {
    return *(VMD_UNIFORM_AS const float*)((VMD_UNIFORM_AS const char*)base + off);
}

template <int VARIANT, unsigned INC, bool SHIFT, class W>
__device__ __forceinline__ void vmd_segment_pruned(const vmd_pair_params_t& p, W& w, vmd_cf32* tx, vmd_cf32* ty, vmd_cf32* tz,
                                                   unsigned ja, unsigned jb, float sx, float sy, float sz,
                                                   float xi, float yi, float zi, const vmd_bbox_t& bb, int lane) {
    const float r2 = p.r2_up;
    const vmd_f2 xi2 = {xi, xi}, yi2 = {yi, yi}, zi2 = {zi, zi};
    const vmd_f2 sx2 = {sx, sx}, sy2 = {sy, sy}, sz2 = {sz, sz};
    // four survivor columns; have < 4: the group is short, the missing columns (which repeat a valid address) are moved out of reach
    auto group = [&](vmd_f4 xj, const vmd_f4& yj, const vmd_f4& zj, int have) {
        if (have < 4) {
            if (have < 2) xj[1] = VMD_FAR;
            if (have < 3) xj[2] = VMD_FAR;
            xj[3] = VMD_FAR;
        }
        vmd_f2 d2[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const vmd_f2 xj2 = {xj[2 * h], xj[2 * h + 1]}, yj2 = {yj[2 * h], yj[2 * h + 1]}, zj2 = {zj[2 * h], zj[2 * h + 1]};
            vmd_f2 dx = xi2 - xj2, dy = yi2 - yj2, dz = zi2 - zj2;
            if (SHIFT) { dx = dx - sx2; dy = dy - sy2; dz = dz - sz2; }
            d2[h] = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
        }
#ifndef VMD_NO_INLINE_ASM
        vmd_push_hot4(w, d2[0][0], d2[0][1], d2[1][0], d2[1][1], r2);
#else
#pragma unroll
        for (int c = 0; c < 4; ++c) vmd_push<VARIANT, INC>(p.bin, w, d2[c >> 1][c & 1] < r2, d2[c >> 1][c & 1]);
#endif
        vmd_drain_full<VARIANT, INC>(p.bin, w, lane);
    };
    // takes up to four survivors off the mask and issues their scalar loads; returns how many were real
    auto fetch = [&](unsigned long long& m, vmd_cf32* px, vmd_cf32* py, vmd_cf32* pz, vmd_f4& xj, vmd_f4& yj, vmd_f4& zj) -> int {
        const int a0 = vmd_sff1(m); m = vmd_sbitclr(m, a0);
        int a1 = vmd_sff1(m); m = vmd_sbitclr(m, a1);
        int a2 = vmd_sff1(m); m = vmd_sbitclr(m, a2);
        int a3 = vmd_sff1(m); m = vmd_sbitclr(m, a3);
        const int have = 1 + (a1 >= 0) + (a2 >= 0) + (a3 >= 0);
        a1 = a1 < 0 ? a0 : a1; a2 = a2 < 0 ? a0 : a2; a3 = a3 < 0 ? a0 : a3;
        const unsigned o0 = 4u * (unsigned)a0, o1 = 4u * (unsigned)a1, o2 = 4u * (unsigned)a2, o3 = 4u * (unsigned)a3;
        xj = vmd_f4{vmd_uniform_load1(px, o0), vmd_uniform_load1(px, o1), vmd_uniform_load1(px, o2), vmd_uniform_load1(px, o3)};
        yj = vmd_f4{vmd_uniform_load1(py, o0), vmd_uniform_load1(py, o1), vmd_uniform_load1(py, o2), vmd_uniform_load1(py, o3)};
        zj = vmd_f4{vmd_uniform_load1(pz, o0), vmd_uniform_load1(pz, o1), vmd_uniform_load1(pz, o2), vmd_uniform_load1(pz, o3)};
        return have;
    };
    // the window after the current one is loaded while the current one is consumed
    auto load = [&](unsigned w0, float& qx, float& qy, float& qz) {
        const unsigned j = w0 + (unsigned)lane;
        const bool valid = j < jb;
        qx = valid ? tx[j] : VMD_FAR; qy = valid ? ty[j] : VMD_FAR; qz = valid ? tz[j] : VMD_FAR;
    };
    float cx, cy, cz;
    load(ja, cx, cy, cz);
    for (unsigned w0 = ja; w0 < jb; w0 += VMD_WAVE) {
        float nx = VMD_FAR, ny = VMD_FAR, nz = VMD_FAR;
        if (w0 + VMD_WAVE < jb) load(w0 + VMD_WAVE, nx, ny, nz);
        float qx = cx, qy = cy, qz = cz;
        if (SHIFT) { qx = qx + sx; qy = qy + sy; qz = qz + sz; }
        const float ex = fmaxf(fmaxf(bb.lox - qx, qx - bb.hix), 0.0f);
        const float ey = fmaxf(fmaxf(bb.loy - qy, qy - bb.hiy), 0.0f);
        const float ez = fmaxf(fmaxf(bb.loz - qz, qz - bb.hiz), 0.0f);
        unsigned long long m = VMD_BALLOT(vmd_d2(ex, ey, ez) <= bb.rp2);      // padding lanes sit at VMD_FAR: never within reach
        vmd_cf32* px = tx + w0;
        vmd_cf32* py = ty + w0;
        vmd_cf32* pz = tz + w0;
        if (m) {
            vmd_f4 xa, ya, za, xb, yb, zb;
            int ha = fetch(m, px, py, pz, xa, ya, za), hb = 0;
            for (;;) {
                const bool more_b = m != 0ull;
                if (more_b) hb = fetch(m, px, py, pz, xb, yb, zb);
                group(xa, ya, za, ha);
                if (!more_b) break;
                const bool more_a = m != 0ull;
                if (more_a) ha = fetch(m, px, py, pz, xa, ya, za);
                group(xb, yb, zb, hb);
                if (!more_a) break;
            }
        }
        cx = nx; cy = ny; cz = nz;
    }
}

// sx == 0 && sy == 0 && sz == 0 for the wave-uniform shifts of a segment, decided from their bit patterns: gfx9 has no scalar float
// compare, the float test is three v_cmp_eq_f32 on 64 lanes for one answer; these are scalar integer instructions.  The shift left drops
// the sign, so -0.0f is zero as in the float test; a NaN is non-zero in both.
__device__ __forceinline__ bool vmd_no_shift(float sx, float sy, float sz) {
    return (((unsigned)__float_as_int(sx) | (unsigned)__float_as_int(sy) | (unsigned)__float_as_int(sz)) << 1) == 0u;
}

template <int VARIANT, unsigned INC, bool MASKED, class W>
__device__ __forceinline__ void vmd_segment(const vmd_pair_params_t& p, W& w, vmd_cf32* st,
                                            unsigned ja, unsigned jb, float sx, float sy, float sz,
                                            float xi, float yi, float zi, unsigned i, unsigned cbeg, int lane) {
    vmd_cf32* tx = st;
    vmd_cf32* ty = st + p.ntgt_pad;
    vmd_cf32* tz = st + 2 * (size_t)p.ntgt_pad;
    // which shifts are not a zero, from their bit patterns on the scalar unit as in vmd_no_shift (both zeros are zero, a NaN is not).  An image
    // of an orthorhombic cell has one live axis unless its pencil wraps in y AND z or it is an x image of a wrapped pencil: a y-wrapped
    // neighbour sy, a z-wrapped one sz, an x image of an unwrapped pencil sx - that loop subtracts one shift per column pair instead of three.
    // Two or three live axes (and every image of a triclinic cell whose sx moves with sy and sz) take the general loop, as does every image
    // of the own pencil's masked part, of the other variants, and of all segments with p.shift_axes == 0 (the A/B switch rdf_shift_axes).
    // (hipcc turns the y and z tests back into v_cmp_eq_f32 against 0; kept from it behind an empty asm they are scalar, eleven scalar
    // instructions more per segment path set, and the kernel is 0.1 ms slower: profiles/pair_loops_ab.txt, state "s")
    const unsigned live = (((unsigned)__float_as_int(sx) << 1) != 0u ? 1u : 0u) | (((unsigned)__float_as_int(sy) << 1) != 0u ? 2u : 0u) |
                          (((unsigned)__float_as_int(sz) << 1) != 0u ? 4u : 0u);
    if (live == 0u) {
        vmd_segment_loop<VARIANT, INC, MASKED, 0>(p, w, tx, ty, tz, ja, jb, sx, sy, sz, xi, yi, zi, i, cbeg, lane);
        return;
    }
    if constexpr (VARIANT == 0 && !MASKED) {
        if (p.shift_axes) {
            if (live == 1u) { vmd_segment_loop<VARIANT, INC, MASKED, 1>(p, w, tx, ty, tz, ja, jb, sx, sy, sz, xi, yi, zi, i, cbeg, lane); return; }
            if (live == 2u) { vmd_segment_loop<VARIANT, INC, MASKED, 2>(p, w, tx, ty, tz, ja, jb, sx, sy, sz, xi, yi, zi, i, cbeg, lane); return; }
            if (live == 4u) { vmd_segment_loop<VARIANT, INC, MASKED, 4>(p, w, tx, ty, tz, ja, jb, sx, sy, sz, xi, yi, zi, i, cbeg, lane); return; }
        }
    }
    vmd_segment_loop<VARIANT, INC, MASKED, 7>(p, w, tx, ty, tz, ja, jb, sx, sy, sz, xi, yi, zi, i, cbeg, lane);
}

// Work distribution: an item is (frame, pencil, sub): the i-chunks sub, sub + nsub, ... of one pencil.  Items are split into
// 8 queues by frame index modulo 8.  A wave first drains the queue of its "home" XCD (blockIdx % 8 — the observed block->XCD
// placement; affinity only, never correctness) so that all pencils of one frame are pulled through ONE XCD's L2, then steals
// from the other queues.  Splitting pencils (nsub > 1) shrinks the number of frames an XCD has in flight (waves / (npen *
// nsub)) so the j streams of the running items stay inside its 4 MiB L2.  Returns the item's index within its frame
// ((pen * nsub + sub) * nsplit + part) and the frame in b, or -1 when every queue is empty (the two halves of the global item id, which
// the kernel used to put together here and divide by nitem_frame again).
// q and tries are wave-uniform and the queue arithmetic (the bound, the frame of the ticket, the id) runs on the scalar unit; only the
// returning atomic is a vector instruction, on lane 0 (until the walk cuts it was all lane 0's: ~30 VALU instructions under a narrowed EXEC
// per item, the division by nitem_frame among them).  vmd_post_item takes a ticket of queue q - it travels while the wave works on the
// current item -, vmd_next_item turns the ticket into an item, or moves on to the next queue when q has run dry (that wait is exposed: at
// most eight times in the life of a wave).  Both are called by all lanes of the wave.
__device__ __forceinline__ unsigned vmd_post_item(unsigned* counters, int q, int tries, int lane) {
    unsigned ticket = 0u;
    if (tries < 8 && lane == 0) ticket = atomicAdd(&counters[q * VMD_COUNTER_STRIDE], 1u);
    return ticket;
}
__device__ __forceinline__ int vmd_next_item(unsigned* counters, unsigned ticket, int& q, int& tries, int B, int nitem_frame, int lane, int& b) {
    while (tries < 8) {
        const unsigned t = (unsigned)__builtin_amdgcn_readfirstlane((int)ticket);
        const int nframes_q = (B - q + 7) >> 3;                 // frames q, q+8, ... < B
        if (nframes_q > 0 && t < (unsigned)(nframes_q * nitem_frame)) {
            const unsigned fq = t / (unsigned)nitem_frame;
            b = q + 8 * (int)fq;
            return (int)(t - fq * (unsigned)nitem_frame);
        }
        q = (q + 1) & 7;
        tries += 1;
        ticket = vmd_post_item(counters, q, tries, lane);
    }
    return -1;
}

// Register budget, rounds 1 - 5 (wave-private histograms): the kernel wants 106 SGPRs (6 waves/SIMD); at 96 a 7th wave fits and the extra
// spills land in the outer (per work item / per segment) loops: +1.7 % on c2 (profiles/r01s_ab.txt).  Round 6: "Occupancy" below.
// TRI: triclinic cell (SPEC S3t).  Pencils and fine cells live in the unsheared coordinates s_k * L_k; a neighbour pencil's
// periodic image is displaced by the lattice vector (kx, nb, nc), and because the Cartesian x of its atoms is
// s_x*Lx + xy*s_y + xz*s_z, the x window is widened by the range that offset takes over the pencil's cross-section.
// CELL = 2: orthorhombic with open axes (non-periodic systems, slabs): an open axis spans the bounding box of the batch (its
// origin sits in the tilt slot of the box record), has no images, and neighbour pencils end at the box.  CELL = 0 is the fully
// periodic orthorhombic cell and carries none of this.
// SHIST: ONE LDS histogram per block (ds_add is atomic across its four waves) instead of one per wave: 10 KB of LDS per block
// instead of 22.5, so 8 blocks = 8 waves per SIMD fit a CU instead of 7.
// Occupancy (round 6): with ONE histogram per block (SHIST: 10 KB of LDS instead of 22.5) eight blocks fit a CU, and the compiler meets the
// register budget of an eighth wave per SIMD (64 VGPRs, 80 SGPRs; 111 instead of 92 SGPRs spilled to VGPR lanes, nothing to scratch) when it
// is told to: c3 71.7 -> 70.4 ms per 1 000 frames, c2 7.35 -> 7.23 (profiles/r06u_eight_waves_ab.txt).  Round 2 had measured the shared
// histogram at seven waves (no gain) and an SGPR cap of 80 on the kernel of that time (no gain); the two together are the default now.
// Wave-private histograms keep the budget of seven waves (96 SGPRs, as capped since round 1: LDS admits no more).
// Neighbour walk: a chunk of 64 i atoms meets the j atoms of its neighbour pencils as segments [ja, jb) of the sorted target copy, one per
// (neighbour pencil, x image) whose x window reaches the chunk.  The segments of a chunk are found by the LANES, not by nested wave-uniform
// loops (gfx9 has no scalar float ALU: every uniform float op ran on the 64-lane VALU for one number, and each segment waited for a
// dependent pair of scalar offset loads; what the table saved is in profiles/segment_table_ab.txt): lane c takes neighbour
// combo c of the (dz, dy) enumeration (dz outer, dy inner; rounds of TABW combos - split pencils 4 x 4 have 81), applies the skip rules
// (half shell, open axis beyond the bounding box, the item's part of an nsplit launch, a shrunk window that vanishes), wraps the pencil and
// derives sy, sz, the shrunk rpad and the triclinic offset range, then for each x image kx = -1, 0, 1 the window [lo, hi], its fine cells and -
// with all loads of the chunk in flight together - ja and jb from the cell offsets.  Everything is the expression, in the order, of the scalar
// walk it replaces.  The entries go to a per-wave LDS table; the walk takes it an x image at a time: the lanes read the image's ja / jb column
// back, one ballot says which entries end in a segment (ja < jb: a lane without a window holds ja == jb), and a scalar loop takes those off
// the mask, brings ja, jb and the shifts of an entry into wave-uniform registers with v_readlane and runs vmd_segment.
// The own pencil is combo (0, 0) = index ry of the half shell.  Segments are walked image by image instead of pencil by pencil: the
// histograms are integer sums.  The table costs 8 KB of LDS per block (5.5 triclinic); with one histogram per block eight blocks still fit a
// CU, with wave-private histograms five do instead of seven.
#ifndef VMD_NO_INLINE_ASM
#define VMD_PENCIL_OCC(SH) __attribute__((amdgpu_waves_per_eu((SH) ? 8 : 7, (SH) ? 8 : 7)))      /* (amdgpu_num_sgpr takes no template-dependent value; seven waves = the cap of 96 SGPRs of rounds 1 - 5) */
#else
#define VMD_PENCIL_OCC(SH)
#endif
// dword offsets into a wave's neighbour segment table of W combo lanes: ja / jb per x image and combo lane, sy / sz per combo lane,
// (triclinic) sx per x image and combo lane
#define VMD_TAB_JA(W) 0
#define VMD_TAB_JB(W) (3 * (W))
#define VMD_TAB_SY(W) (6 * (W))
#define VMD_TAB_SZ(W) (7 * (W))
#define VMD_TAB_SX(W) (8 * (W))
template <int VARIANT_, bool SAME, int CELL, bool SHIST, int POP = 0>
__global__ __launch_bounds__(256) VMD_PENCIL_OCC(SHIST) void k_rdf_pencil(vmd_pair_params_t p) {
    constexpr bool TRI = CELL == 1, OPEN = CELL == 2;
    constexpr bool PRUNE = VARIANT_ == 3;            // variant 3 = variant 0 + bounding-box pruning of the j windows
    constexpr int VARIANT = PRUNE ? 0 : VARIANT_;
    __shared__ unsigned s_hist[SHIST ? 1 : 4][VMD_MAX_BINS + 2];       // + the spare bin of vmd_pop_hot0 (index nbins; never read)
    // (looking at the stack once per EIGHT columns - a 640-float stack, which the one-histogram kernels have the LDS for - measured 1 % slower
    // than once per four: profiles/r06v_salu_ab.txt)
    __shared__ float s_queue[4][VMD_QUEUE_CAP];
    // the wave's neighbour segment table (one round of combos).  A triclinic cell also keeps sx per entry and takes its rounds on 32 lanes, so
    // that histogram, stack and table of eight blocks still fit a CU (5.5 KB and 8 KB of table per block)
    constexpr int TABW = TRI ? 32 : VMD_WAVE;
    __shared__ unsigned s_tab[4][(TRI ? 11 : 8) * TABW];
    constexpr unsigned INC = SAME ? 2u : 1u;
    if (p.skip && *p.skip) return;       // set before this launch by the cell build; the host repeats the batch with larger buckets

    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int nbins = p.bin.nbins;

    vmd_wave_acc_tt<POP> w;
    w.hist = s_hist[SHIST ? 0 : wave];
    w.queue = s_queue[wave];
    w.qbase = VMD_LDS_ADDRESS(s_queue[wave]);
    w.hbase = VMD_LDS_ADDRESS(s_hist[SHIST ? 0 : wave]);
    w.qtop = w.qbase;
    w.qlim = w.qbase + 4u * VMD_WAVE;
    w.slow = &s_queue[wave][VMD_QUEUE_CAP - VMD_WAVE];
    w.nslow = 0;
    w.fast_c = vmd_in_vgpr(p.bin.fast_c);
    w.fast_k = vmd_in_vgpr(p.bin.fast_k);
    w.fast_far = vmd_in_vgpr(p.bin.fast_far);
    w.fast_c2 = vmd_in_vgpr(p.bin.fast_c2);
    w.ncols = 0;
    if (SHIST) {
        for (int b = threadIdx.x; b < nbins; b += 256) s_hist[0][b] = 0u;
        __syncthreads();
    } else {
        for (int b = lane; b < nbins; b += VMD_WAVE) w.hist[b] = 0u;
        __builtin_amdgcn_wave_barrier();
    }

    const int nxf = p.grid.nxf, ny = p.grid.ny, nz = p.grid.nz;
    const int npen = ny * nz;

    unsigned long long cols_before_flush = 0ull;
    // work items are handed out dynamically (one returning atomic per item, fetched one item ahead)
    int q = blockIdx.x & 7, tries = 0;
    const int nsub = p.nsub;
    const int nsplit = p.nsplit;
    const int nitem_frame = npen * nsub * nsplit;
    // neighbour combos (dz, dy) in the order dz outer, dy inner; the same-set half shell starts at dz = 0 and drops dy < 0 there
    const int ncy = 2 * p.ry + 1, dz0 = SAME ? 0 : -p.rz;
    const int ncombo = (p.rz - dz0 + 1) * ncy;
    const int cdiv = 65536 / ncy + 1;                       // (c * cdiv) >> 16 == c / ncy for c * ncy < 65536 (the reach is at most 4: 81 combos)
    unsigned* tab = s_tab[wave];
    // reach 1 in both axes (every unsplit grid): no window ever shrinks, and the pencil widths the shrink needs - two IEEE divisions, which
    // the compiler otherwise hoists out of the table to the item and runs for every chunk - are not computed at all
    const bool split = CELL == 0 && (p.ry > 1 || p.rz > 1);
    unsigned ticket = vmd_post_item(p.work_counter, q, tries, lane);
    int b = 0;
    int rem0 = vmd_next_item(p.work_counter, ticket, q, tries, p.B, nitem_frame, lane, b);
    while (rem0 >= 0) {
        ticket = vmd_post_item(p.work_counter, q, tries, lane);
        // (nothing here is negative: unsigned divisions, which cost the scalar unit a third less than signed ones)
        const int rem = (int)((unsigned)rem0 / (unsigned)nsplit);
        const int part = rem0 - rem * nsplit;               // which of the chunk's neighbour pencils this item walks (fastest: the parts of
        const int pen = (int)((unsigned)rem / (unsigned)nsub);      // a chunk go to consecutive waves, which share its i atoms and its neighbourhood)
        const int sub = rem - pen * nsub;
        const int pz = (int)((unsigned)pen / (unsigned)ny);
        const int py = pen - pz * ny;
        vmd_cf32* boxes = (vmd_cf32*)p.boxes;
        // the box edges are operands of the table's lanes: held in a VGPR each for the item.  As scalars they were parked in VGPR lanes as the
        // four-dword tuple of their load, and every use in the table round and the image loop read all four lanes back
        const float Lx = vmd_in_vgpr(boxes[VMD_BOX_STRIDE * b + 0]), Ly = vmd_in_vgpr(boxes[VMD_BOX_STRIDE * b + 1]),
                    Lz = vmd_in_vgpr(boxes[VMD_BOX_STRIDE * b + 2]);
        const float inv_cx = (float)nxf * boxes[VMD_BOX_STRIDE * b + 3];
        float wy = 0.0f, wz = 0.0f;                         // the frame's pencil widths, split grids only
        if (split) { wy = Ly / vmd_pin((float)ny); wz = Lz / vmd_pin((float)nz); }      // (pinned: else both divisions run ahead of the branch, behind two selects)
        const float txy = TRI ? boxes[VMD_BOX_STRIDE * b + 6] : 0.0f, txz = TRI ? boxes[VMD_BOX_STRIDE * b + 7] : 0.0f,
                    tyz = TRI ? boxes[VMD_BOX_STRIDE * b + 8] : 0.0f;
        // open x axis: fine cells count from the bounding-box origin (0 on a periodic axis)
        const bool open_x = OPEN && !(p.pbc & 1u), open_y = OPEN && !(p.pbc & 2u), open_z = OPEN && !(p.pbc & 4u);
        const float orgx = open_x ? boxes[VMD_BOX_STRIDE * b + 6] : 0.0f;
        // open x axis: coordinates are not wrapped, so x - origin is rounded at the magnitude of the raw coordinate, in the
        // build and again here; widen the window by a few such ulps (a system far from the origin must not lose a boundary pair)
        const float pad_open = open_x ? 8.0e-7f * (fabsf(orgx) + Lx) : 0.0f;
        vmd_cu32* csr = (vmd_cu32*)p.cs_ref + (size_t)b * (p.grid.ncell + 1);
        vmd_cu32* cst = (vmd_cu32*)p.cs_tgt + (size_t)b * (p.grid.ncell + 1);
        const float* __restrict__ sr = p.sref + (size_t)b * 3 * p.nref_pad;
        vmd_cf32* st = (vmd_cf32*)p.stgt + (size_t)b * 3 * p.ntgt_pad;
        const unsigned pbeg = csr[pen * nxf];
        const unsigned pend = csr[(pen + 1) * nxf];

        for (unsigned cbeg = pbeg + (unsigned)sub * VMD_WAVE; cbeg < pend; cbeg += (unsigned)nsub * VMD_WAVE) {
            const unsigned i = cbeg + lane;
            const bool valid = i < pend;
            const float xi = valid ? sr[i] : VMD_FAR;
            const float yi = valid ? sr[p.nref_pad + i] : VMD_FAR;
            const float zi = valid ? sr[2 * (size_t)p.nref_pad + i] : VMD_FAR;
            const float xlo = vmd_wave64_min(valid ? xi : 3.0e38f);
            const float xhi = vmd_wave64_max(valid ? xi : -3.0e38f);
            vmd_bbox_t bb = {};
            if (PRUNE) {
                bb.lox = xlo; bb.hix = xhi;
                bb.loy = vmd_wave64_min(valid ? yi : 3.0e38f); bb.hiy = vmd_wave64_max(valid ? yi : -3.0e38f);
                bb.loz = vmd_wave64_min(valid ? zi : 3.0e38f); bb.hiz = vmd_wave64_max(valid ? zi : -3.0e38f);
                // reach of the box test: the padded cutoff + the rounding of coordinates of this magnitude (images included)
                const float mag = fmaxf(fmaxf(fmaxf(fabsf(bb.lox), fabsf(bb.hix)), fmaxf(fabsf(bb.loy), fabsf(bb.hiy))), fmaxf(fabsf(bb.loz), fabsf(bb.hiz)))
                                  + Lx + Ly + Lz + fabsf(txy) + fabsf(txz) + fabsf(tyz);
                const float rp = p.rpad + 4.0e-6f * mag;
                bb.rp2 = rp * rp;
            }

            // the neighbour table: lane c of a round takes combo c0 + c, all three x images of it
            for (int c0 = 0; c0 < ncombo; c0 += TABW) {
                const int c = c0 + lane;
                const int dzi = (c * cdiv) >> 16;                   // c / ncy
                const int dz = dz0 + dzi, dy = c - dzi * ncy - p.ry;
                bool ok = c < ncombo && lane < TABW;
                int qz = pz + dz; float sz = 0.0f, nc = 0.0f;
                if (open_z && (qz < 0 || qz >= nz)) ok = false;     // nothing beyond the bounding box
                if (qz < 0) { qz += nz; sz = -Lz; nc = -1.0f; } else if (qz >= nz) { qz -= nz; sz = Lz; nc = 1.0f; }
                if (SAME && dz == 0 && dy < 0) ok = false;
                if (nsplit > 1 && ((dz + p.rz) * ncy + (dy + p.ry)) % nsplit != part) ok = false;
                int qy = py + dy; float sy = 0.0f, nb = 0.0f;
                if (open_y && (qy < 0 || qy >= ny)) ok = false;
                if (qy < 0) { qy += ny; sy = -Ly; nb = -1.0f; } else if (qy >= ny) { qy -= ny; sy = Ly; nb = 1.0f; }
                const int q = qz * ny + qy;
                float offmin = 0.0f, offmax = 0.0f;
                // split pencils: a neighbour two pencils away is at least one pencil width off in that axis, so its x window shrinks
                // (orthorhombic periodic cells only; the widths of the other cell kinds are not the box edge over the count)
                float rpad = p.rpad;
                if (split && (dy > 1 || dy < -1 || dz > 1 || dz < -1)) {          // (split: wave-uniform, a scalar branch around the block)
                    const float gy = (float)((dy < 0 ? -dy : dy) - 1) * wy, gz = (float)((dz < 0 ? -dz : dz) - 1) * wz;
                    const float gyy = gy > 0.0f ? gy : 0.0f, gzz = gz > 0.0f ? gz : 0.0f;
                    const float rr = p.rpad * p.rpad - 0.998f * (gyy * gyy + gzz * gzz);
                    if (rr <= 0.0f) ok = false;
                    rpad = sqrtf(rr) * 1.0001f;
                }
                if (TRI) {
                    // range of xy*s_y + xz*s_z over the cross-section of pencil q (+ head room for the roundings)
                    const float fny = vmd_uniform((float)ny), fnz = vmd_uniform((float)nz);      // (wave-uniform: not held in a VGPR across the segments)
                    const float y0 = txy * ((float)qy / fny), y1 = txy * ((float)(qy + 1) / fny);
                    const float z0 = txz * ((float)qz / fnz), z1 = txz * ((float)(qz + 1) / fnz);
                    offmin = fminf(y0, y1) + fminf(z0, z1) - 1.0e-3f;
                    offmax = fmaxf(y0, y1) + fmaxf(z0, z1) + 1.0e-3f;
                }
                // (CELL == 0 at reach 1: lo, hi, ca, cb of an image depend on xlo, xhi and kx only, not on the combo lane.  The compiler shares
                // (xlo - rpad) and (xhi + rpad) across the three unrolled images and folds the TRI / OPEN zeros; what is left per image - one
                // subtraction, two compares, two vmd_cell_coord - costs a VALU instruction the same for one value as for 64 lanes.)
                unsigned ia[3], ib[3];                              // (never negative; unsigned: the lanes' load addresses need no sign extension)
                bool in[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int kx = k - 1;
                    float sx = (float)kx * Lx;
                    if (TRI) vmd_lattice_shift(Lx, Ly, Lz, txy, txz, tyz, (float)kx, nb, nc, sx, sy, sz);      // sy, sz: the same for every kx
                    const float lo = (xlo - rpad) - sx - offmax - orgx - pad_open;
                    const float hi = (xhi + rpad) - sx - offmin - orgx + pad_open;
                    in[k] = ok && !(open_x && kx != 0) && !(hi < 0.0f || lo >= Lx);
                    const int ca = lo <= 0.0f ? 0 : vmd_cell_coord(lo, inv_cx, nxf);
                    const int cb = hi >= Lx ? nxf - 1 : vmd_cell_coord(hi, inv_cx, nxf);
                    ia[k] = in[k] ? (unsigned)(q * nxf + ca) : 0u;  // (a lane without a window reads cst[0]: always there)
                    ib[k] = in[k] ? (unsigned)(q * nxf + cb + 1) : 0u;
                    if (TRI && lane < TABW) tab[VMD_TAB_SX(TABW) + k * TABW + lane] = (unsigned)__float_as_int(sx);
                }
                // all of the chunk's offsets travel together
                const unsigned ja0 = cst[ia[0]], jb0 = cst[ib[0]], ja1 = cst[ia[1]], jb1 = cst[ib[1]], ja2 = cst[ia[2]], jb2 = cst[ib[2]];
                if (lane < TABW) {
                    tab[VMD_TAB_JA(TABW) + lane] = ja0; tab[VMD_TAB_JA(TABW) + TABW + lane] = ja1; tab[VMD_TAB_JA(TABW) + 2 * TABW + lane] = ja2;
                    tab[VMD_TAB_JB(TABW) + lane] = jb0; tab[VMD_TAB_JB(TABW) + TABW + lane] = jb1; tab[VMD_TAB_JB(TABW) + 2 * TABW + lane] = jb2;
                    tab[VMD_TAB_SY(TABW) + lane] = (unsigned)__float_as_int(sy); tab[VMD_TAB_SZ(TABW) + lane] = (unsigned)__float_as_int(sz);
                }
                __builtin_amdgcn_wave_barrier();
                // The walk takes the table an image at a time: the lanes read the image's ja / jb column back (and once per round the sy / sz
                // column) and a segment's entry comes out of those registers with v_readlane.  Per SEGMENT it used to be two LDS reads at a
                // wave-uniform address built in a VGPR and four v_readfirstlane behind their latency; the three ballots of a round were parked
                // in VGPR lanes and all six halves read back for every image.
                const unsigned lsy = lane < TABW ? tab[VMD_TAB_SY(TABW) + lane] : 0u, lsz = lane < TABW ? tab[VMD_TAB_SZ(TABW) + lane] : 0u;
#pragma unroll 1
                for (int k = 0; k < 3; ++k) {
                    const unsigned lja = lane < TABW ? tab[VMD_TAB_JA(TABW) + k * TABW + lane] : 0u, ljb = lane < TABW ? tab[VMD_TAB_JB(TABW) + k * TABW + lane] : 0u;
                    const unsigned lsx = TRI && lane < TABW ? tab[VMD_TAB_SX(TABW) + k * TABW + lane] : 0u;
                    // the entries that end in a segment (an own pencil's two parts are both empty when ja >= jb).  A lane without a window has
                    // read cst[0] twice, ja == jb: the compare alone is the ballot
                    unsigned long long m = VMD_BALLOT(lja < ljb);
                    const unsigned lxb = (unsigned)__float_as_int(vmd_uniform(Lx));      // (read per image: one v_readfirstlane, no parked SGPR)
                    // (float)(k - 1) * Lx of a finite Lx, from its bit pattern on the scalar unit: -Lx, a zero with the sign of Lx, Lx
                    // (on the vector unit it was a subtract, a convert, a multiply and a v_readfirstlane per image)
                    const float sxk = __int_as_float((int)(k == 0 ? lxb ^ 0x80000000u : (k == 1 ? lxb & 0x80000000u : lxb)));
                    while (m) {
                        const int e = __builtin_ctzll(m);
                        m &= m - 1ull;
                        unsigned ja = VMD_READLANE_U32(lja, e);
                        const unsigned jb = VMD_READLANE_U32(ljb, e);
                        const float sx = TRI ? __int_as_float((int)VMD_READLANE_U32(lsx, e)) : sxk;
                        const float sy = __int_as_float((int)VMD_READLANE_U32(lsy, e));
                        const float sz = __int_as_float((int)VMD_READLANE_U32(lsz, e));
                        if (SAME && c0 + e == p.ry) {               // the own pencil: combo (dz, dy) = (0, 0)
                            // unordered pairs once: j > i.  Inside the chunk the test is per lane, above it all lanes pass.
                            const unsigned cend = cbeg + VMD_WAVE;
                            const unsigned ma = ja > cbeg ? ja : cbeg;
                            const unsigned mb = jb < cend ? jb : cend;
                            if (ma < mb) {
                                w.ncols += mb - ma;
                                vmd_segment<VARIANT, INC, true>(p, w, st, ma, mb, sx, sy, sz, xi, yi, zi, i, cbeg, lane);
                            }
                            ja = ja > cend ? ja : cend;
                        }
                        if (ja < jb) {
                            w.ncols += jb - ja;
                            if (PRUNE) {
                                vmd_cf32* tx = st; vmd_cf32* ty = st + p.ntgt_pad; vmd_cf32* tz = st + 2 * (size_t)p.ntgt_pad;
                                if (vmd_no_shift(sx, sy, sz)) vmd_segment_pruned<VARIANT, INC, false>(p, w, tx, ty, tz, ja, jb, sx, sy, sz, xi, yi, zi, bb, lane);
                                else vmd_segment_pruned<VARIANT, INC, true>(p, w, tx, ty, tz, ja, jb, sx, sy, sz, xi, yi, zi, bb, lane);
                            } else {
                                vmd_segment<VARIANT, INC, false>(p, w, st, ja, jb, sx, sy, sz, xi, yi, zi, i, cbeg, lane);
                            }
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();                    // the table is read out before the next round overwrites it
            }
            // u32 LDS counters: every candidate column adds at most 64*INC; flush long before 2^32 (rare: straight to the
            // device accumulators with atomics)
            // (a shared histogram receives the columns of four waves: a quarter of the budget each, and the flush takes the bins
            // with an atomic exchange - an increment of another wave lands either before it, and travels now, or after it, and stays)
            if (w.ncols >= (SHIST ? (1u << 21) : (1u << 23))) {
                cols_before_flush += w.ncols;
                vmd_drain<VARIANT, INC>(p.bin, w, lane);
                __builtin_amdgcn_wave_barrier();
                for (int bb = lane; bb < nbins; bb += VMD_WAVE) {
                    const unsigned v = SHIST ? atomicExch(&w.hist[bb], 0u) : w.hist[bb];
                    if (v) atomicAdd(&p.counts[bb], (unsigned long long)v);
                    if (!SHIST) w.hist[bb] = 0u;
                }
                __builtin_amdgcn_wave_barrier();
                w.ncols = 0;
            }
        }
        rem0 = vmd_next_item(p.work_counter, ticket, q, tries, p.B, nitem_frame, lane, b);
    }
    vmd_drain<VARIANT, INC>(p.bin, w, lane);
    if (p.cols_total && lane == 0) atomicAdd(p.cols_total, cols_before_flush + (unsigned long long)w.ncols);
    // one row per block: the four wave histograms are summed through LDS and stored with plain, coalesced writes
    __syncthreads();
    uint64_t* __restrict__ prow = p.partial + (size_t)blockIdx.x * nbins;
    for (int bb = threadIdx.x; bb < nbins; bb += 256) {
        uint64_t v = s_hist[0][bb];
        if (!SHIST) v = v + s_hist[1][bb] + s_hist[2][bb] + s_hist[3][bb];
        prow[bb] = v;
    }
}

// sum the per-block partial rows into the u64 accumulators: block (x = 256 bins, y = slice of 32 rows), coalesced
// row reads, one atomicAdd(u64) per bin and slice
__global__ __launch_bounds__(256) void k_hist_reduce(const uint64_t* __restrict__ partial, int nrows, int nbins,
                                                     uint64_t* __restrict__ counts, const uint32_t* __restrict__ skip) {
    if (skip && *skip) return;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nbins) return;
    const int r0 = blockIdx.y * 32;
    const int r1 = r0 + 32 < nrows ? r0 + 32 : nrows;
    uint64_t s = 0;
    for (int r = r0; r < r1; ++r) s += partial[(size_t)r * nbins + b];
    if (s) atomicAdd((unsigned long long*)&counts[b], (unsigned long long)s);
}

// ------------------------------------------------------------------------------------------------ RDF, general (brute)

struct vmd_brute_params_t {
    const float* xyz; size_t frame_stride; size_t row_stride;
    const float* boxes; uint32_t pbc; int B;
    const int32_t* ref; int nref; const int32_t* tgt; int ntgt;
    vmd_binning_t bin;
    uint64_t* counts;
    int raw;            // DECISION(D-WRAP) flipped: positions as they are, minimum image by rounding (oracle: vo_set_spec("rdf_raw", 1))
    const unsigned char* mref; const unsigned char* mtgt;     // MASKED: u8[B][nref] / u8[B][ntgt] per-frame masks, NULL = all
};

// MASKED: list entries whose byte is 0 take no part in that frame - a shell where no grid exists
template <bool MASKED>
__global__ __launch_bounds__(256) void k_rdf_brute(vmd_brute_params_t p) {
    __shared__ unsigned s_hist[VMD_MAX_BINS];
    __shared__ float s_t[3][256];
    __shared__ unsigned char s_m[MASKED ? 256 : 1];
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const float* fx = p.xyz + (size_t)b * p.frame_stride;
    const float* fy = fx + p.row_stride;
    const float* fz = fy + p.row_stride;
    const vmd_box_t bx = vmd_load_box(p.boxes, b, p.pbc);
    for (int k = threadIdx.x; k < p.bin.nbins; k += 256) s_hist[k] = 0u;
    float xi = VMD_FAR, yi = VMD_FAR, zi = VMD_FAR;
    bool valid = t < p.nref;
    if (MASKED) { if (valid && p.mref) valid = p.mref[(size_t)b * p.nref + t] != 0; }
    if (valid) {
        const int a = p.ref ? p.ref[t] : t;
        if (p.raw) { xi = fx[a]; yi = fy[a]; zi = fz[a]; }
        else vmd_pair_coords(bx, fx[a], fy[a], fz[a], xi, yi, zi);
    }
    for (int j0 = 0; j0 < p.ntgt; j0 += 256) {
        __syncthreads();
        const int j = j0 + threadIdx.x;
        if (j < p.ntgt) {
            const int a = p.tgt ? p.tgt[j] : j;
            if (p.raw) { s_t[0][threadIdx.x] = fx[a]; s_t[1][threadIdx.x] = fy[a]; s_t[2][threadIdx.x] = fz[a]; }
            else vmd_pair_coords(bx, fx[a], fy[a], fz[a], s_t[0][threadIdx.x], s_t[1][threadIdx.x], s_t[2][threadIdx.x]);
            if (MASKED) s_m[threadIdx.x] = p.mtgt ? p.mtgt[(size_t)b * p.ntgt + j] : 1;
        }
        __syncthreads();
        const int nj = p.ntgt - j0 < 256 ? p.ntgt - j0 : 256;
        if (valid) {
            for (int jj = 0; jj < nj; ++jj) {
                if (MASKED) { if (!s_m[jj]) continue; }
                float d2;
                if (p.raw && !bx.tri) {
                    float dx = xi - s_t[0][jj], dy = yi - s_t[1][jj], dz = zi - s_t[2][jj];
                    dx = vmd_mi_rintf(dx, bx.Lx, bx.iLx, bx.px); dy = vmd_mi_rintf(dy, bx.Ly, bx.iLy, bx.py); dz = vmd_mi_rintf(dz, bx.Lz, bx.iLz, bx.pz);
                    d2 = vmd_d2(dx, dy, dz);
                } else d2 = vmd_pair_d2_general(bx, xi, yi, zi, s_t[0][jj], s_t[1][jj], s_t[2][jj]);      // S3t takes positions as they come
                const int bin = vmd_bin_of(p.bin, d2);
                if (bin >= 0) atomicAdd(&s_hist[bin], 1u);
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < p.bin.nbins; k += 256) {
        const unsigned v = s_hist[k];
        if (v) atomicAdd((unsigned long long*)&p.counts[k], (unsigned long long)v);
    }
}

// ------------------------------------------------------------------------------------------------ K6: within

// count(T and within(r_min:r_max, R)): target t is in iff SOME reference atom lies at r_min <= d < r_max (closed: d <= r_max), d the
// correctly rounded sqrtf of the S3 / S3t squared distance - the d vmd_bin_of bins.  r2_up is a coarse bound in front of the root: every
// d2 whose root can be <= r_max lies below it (+inf where r_max^2 leaves the normal range: the root decides alone).
struct vmd_within_test_t { float rmin, rmax, r2_up; int closed; };
static inline vmd_within_test_t vmd_make_within_test(float rmin, float rmax, int closed) {
    vmd_within_test_t w;
    w.rmin = rmin; w.rmax = rmax; w.closed = closed ? 1 : 0;
    const float r2 = rmax * rmax;
    w.r2_up = (r2 > 1.0e-30f && r2 < 1.0e30f) ? nextafterf(r2, 3.0e38f) * 1.0001f : INFINITY;
    return w;
}
__device__ __forceinline__ bool vmd_within_hit(const vmd_within_test_t& w, float d2) {
    if (!(d2 < w.r2_up)) return false;
    const float d = sqrtf(d2);
    return w.rmin <= d && (w.closed ? d <= w.rmax : d < w.rmax);
}

struct vmd_within_brute_params_t {
    const float* xyz; size_t frame_stride; size_t row_stride;
    const float* boxes; uint32_t pbc; int B;
    const int32_t* tgt; int ntgt; const int32_t* ref; int nref;
    vmd_within_test_t w;
    unsigned* count;
    unsigned char* flags;       // FLAGS instantiation: u8[B][ntgt], 1 = the list entry is in the shell
    size_t flag_stride;         // ATOMS instantiation: flags is u8[B][flag_stride] indexed by ATOM, flags[b][tgt[t]]
};

// All pairs from the raw frame (any cell, any cutoff), the one tile loop of every all-pairs kernel: one lane per atom at the wrapped position
// (xi, yi, zi) (`active` false: a lane without one), the list (nullptr: every atom) staged through the caller's LDS tile 256 entries at a
// time by the block's NT threads, from tile `first` on (block-uniform; 0 but for an upper triangle).  stage(slot, pos) runs for every
// entry as it is staged, between the same two barriers, and fills the kernel's own LDS columns; visit(slot, pos, ex, ey, ez) runs in the
// lane for every staged entry, e = (lane - entry) - shift of the S3 / S3t image, and returns true when the lane has seen enough (-> true).
// Every thread of the block calls it: two barriers per tile.
template <int NT, class Stage, class Visit>
__device__ __forceinline__ bool vmd_all_pairs(float (&s_r)[3][256], const vmd_box_t& bx, const float* fx, const float* fy, const float* fz,
        const int32_t* list, int n, int first, bool active, float xi, float yi, float zi, Stage stage, Visit visit) {
    bool stop = false;
    for (int j0 = first; j0 < n; j0 += 256) {
        __syncthreads();
        const int nj = n - j0 < 256 ? n - j0 : 256;
        for (int jj = threadIdx.x; jj < nj; jj += NT) {
            const int a = list ? list[j0 + jj] : j0 + jj;
            vmd_pair_coords(bx, fx[a], fy[a], fz[a], s_r[0][jj], s_r[1][jj], s_r[2][jj]);
            stage(jj, j0 + jj);
        }
        __syncthreads();
        if (active && !stop)
            for (int jj = 0; jj < nj && !stop; ++jj) {
                float ex, ey, ez;
                vmd_pair_delta_general(bx, xi, yi, zi, s_r[0][jj], s_r[1][jj], s_r[2][jj], ex, ey, ez);
                stop = visit(jj, j0 + jj, ex, ey, ez);
            }
    }
    return stop;
}

// within() by all pairs, the device-side definition the cell walk below is tested against: a lane stops testing at its first hit
template <int NT>
__device__ __forceinline__ bool vmd_within_all_pairs(float (&s_r)[3][256], const vmd_box_t& bx, const float* fx, const float* fy,
        const float* fz, const int32_t* ref, int nref, const vmd_within_test_t& w, bool active, float xi, float yi, float zi) {
    return vmd_all_pairs<NT>(s_r, bx, fx, fy, fz, ref, nref, 0, active, xi, yi, zi, [](int, int) {},
                             [&](int, int, float ex, float ey, float ez) { return vmd_within_hit(w, vmd_d2(ex, ey, ez)); });
}

// One lane per target atom over vmd_within_all_pairs, one integer atomic per wave.
// FLAGS: also one byte per list entry, in list order - the mask vmd_hip_rdf_brute_masked takes.
// ATOMS (with FLAGS): the byte goes to the atom's place instead, the mask vmd_hip_sdf_scatter_masked takes where no grid exists.
template <bool FLAGS, bool ATOMS = false>
__global__ __launch_bounds__(256) void k_within_brute(vmd_within_brute_params_t p) {
    __shared__ float s_r[3][256];
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const float* fx = p.xyz + (size_t)b * p.frame_stride;
    const float* fy = fx + p.row_stride;
    const float* fz = fy + p.row_stride;
    const vmd_box_t bx = vmd_load_box(p.boxes, b, p.pbc);
    float xi = VMD_FAR, yi = VMD_FAR, zi = VMD_FAR;
    const bool valid = t < p.ntgt;
    if (valid) {
        const int a = p.tgt ? p.tgt[t] : t;
        vmd_pair_coords(bx, fx[a], fy[a], fz[a], xi, yi, zi);
    }
    const bool hit = vmd_within_all_pairs<256>(s_r, bx, fx, fy, fz, p.ref, p.nref, p.w, valid, xi, yi, zi);
    if (FLAGS && ATOMS) { if (valid) p.flags[(size_t)b * p.flag_stride + (size_t)(p.tgt ? p.tgt[t] : t)] = hit ? 1 : 0; }
    else if (FLAGS) { if (valid) p.flags[(size_t)b * p.ntgt + t] = hit ? 1 : 0; }
    const unsigned long long m = __ballot(hit ? 1 : 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&p.count[b], (unsigned)__popcll(m));
}

// the cell walk's part of a kernel's parameters, as vmd_within_walk_fill writes it ...
struct vmd_within_walk_params_t {
    const float* sref; const uint32_t* cs_ref; int nref_pad;      // the sorted copy of R and its cell_start
    vmd_within_test_t w; float rpad;                              // rpad: the padded window, > rmax
    int ry, rz;                                                   // neighbour pencils either way (1; 2 with split pencils)
};

// ... and what a block derives from it for its frame b, once (vmd_within_walk_setup)
struct vmd_within_walk_t {
    int nxf, ny, nz;
    bool tri, open, open_x, open_y, open_z;
    float Lx, Ly, Lz, inv_cx, txy, txz, tyz, orgx, pad_open, rpad;
    int ry, rz;
    const uint32_t* csr; const float *xr, *yr, *zr;               // frame b's cell_start and coordinate rows of the sorted copy
    vmd_within_test_t w;
};

__device__ __forceinline__ vmd_within_walk_t vmd_within_walk_setup(const float* boxes, int b, uint32_t pbc, const vmd_grid_t& grid,
        const vmd_within_walk_params_t& p) {
    vmd_within_walk_t k;
    k.nxf = grid.nxf; k.ny = grid.ny; k.nz = grid.nz;
    k.tri = (pbc & VMD_PBC_TRICLINIC) != 0; k.open = !k.tri && (pbc & 7u) != 7u;
    const float* q = boxes + (size_t)VMD_BOX_STRIDE * b;
    k.Lx = q[0]; k.Ly = q[1]; k.Lz = q[2];
    k.inv_cx = (float)k.nxf * q[3];
    k.txy = k.tri ? q[6] : 0.0f; k.txz = k.tri ? q[7] : 0.0f; k.tyz = k.tri ? q[8] : 0.0f;
    k.open_x = k.open && !(pbc & 1u); k.open_y = k.open && !(pbc & 2u); k.open_z = k.open && !(pbc & 4u);
    k.orgx = k.open_x ? q[6] : 0.0f;
    k.pad_open = k.open_x ? 8.0e-7f * (fabsf(k.orgx) + k.Lx) : 0.0f;
    k.rpad = p.rpad; k.ry = p.ry; k.rz = p.rz;
    k.csr = p.cs_ref + (size_t)b * (grid.ncell + 1);
    k.xr = p.sref + (size_t)b * 3 * p.nref_pad;
    k.yr = k.xr + p.nref_pad;
    k.zr = k.yr + p.nref_pad;
    k.w = p.w;
    return k;
}

// The cell walk: which members of R are in range of the atom at (xi, yi, zi), standing in pencil (py, pz) of the grid?  R comes cell-sorted
// (K1), so the x window [x - r, x + r] of a neighbour pencil is one run of the sorted copy per periodic image; pencils, images, window
// arithmetic and the pair arithmetic are those of k_rdf_pencil (the neighbour cell's image is the comparison's for every d < r_max), with
// the window of ONE atom instead of a chunk's.  visit(slot, ex, ey, ez) for every member that passes vmd_within_hit, e = (atom - member) -
// shift; it returns true when the lane has seen enough, and the lane leaves the walk (-> true).  A pair is met under one image only: a grid exists
// only where the minimum image is unique for every hit (choose_grid), so the other images of a slot fail the distance.
template <class Visit>
__device__ __forceinline__ bool vmd_within_walk_each(const vmd_within_walk_t& k, int py, int pz, float xi, float yi, float zi, Visit visit) {
    bool stop = false;
    for (int dz = -k.rz; dz <= k.rz && !stop; ++dz) {
        int qz = pz + dz; float sz = 0.0f, nc = 0.0f;
        if (k.open_z && (qz < 0 || qz >= k.nz)) continue;
        if (qz < 0) { qz += k.nz; sz = -k.Lz; nc = -1.0f; } else if (qz >= k.nz) { qz -= k.nz; sz = k.Lz; nc = 1.0f; }
        for (int dy = -k.ry; dy <= k.ry && !stop; ++dy) {
            int qy = py + dy; float sy = 0.0f, nb = 0.0f;
            if (k.open_y && (qy < 0 || qy >= k.ny)) continue;
            if (qy < 0) { qy += k.ny; sy = -k.Ly; nb = -1.0f; } else if (qy >= k.ny) { qy -= k.ny; sy = k.Ly; nb = 1.0f; }
            const int qp = qz * k.ny + qy;
            float offmin = 0.0f, offmax = 0.0f, rpad = k.rpad;
            if (!k.tri && !k.open && (dy > 1 || dy < -1 || dz > 1 || dz < -1)) {      // split pencils: the outer ones see a shorter window
                const float gy = (float)((dy < 0 ? -dy : dy) - 1) * (k.Ly / (float)k.ny), gz = (float)((dz < 0 ? -dz : dz) - 1) * (k.Lz / (float)k.nz);
                const float gyy = gy > 0.0f ? gy : 0.0f, gzz = gz > 0.0f ? gz : 0.0f;
                const float rr = k.rpad * k.rpad - 0.998f * (gyy * gyy + gzz * gzz);
                if (rr <= 0.0f) continue;
                rpad = sqrtf(rr) * 1.0001f;
            }
            if (k.tri) {
                const float y0 = k.txy * ((float)qy / (float)k.ny), y1 = k.txy * ((float)(qy + 1) / (float)k.ny);
                const float z0 = k.txz * ((float)qz / (float)k.nz), z1 = k.txz * ((float)(qz + 1) / (float)k.nz);
                offmin = fminf(y0, y1) + fminf(z0, z1) - 1.0e-3f;
                offmax = fmaxf(y0, y1) + fmaxf(z0, z1) + 1.0e-3f;
            }
            for (int kx = -1; kx <= 1 && !stop; ++kx) {
                if (k.open_x && kx != 0) continue;
                float sx = (float)kx * k.Lx, sy2 = sy, sz2 = sz;
                if (k.tri) vmd_lattice_shift(k.Lx, k.Ly, k.Lz, k.txy, k.txz, k.tyz, (float)kx, nb, nc, sx, sy2, sz2);
                const float lo = (xi - rpad) - sx - offmax - k.orgx - k.pad_open;
                const float hi = (xi + rpad) - sx - offmin - k.orgx + k.pad_open;
                if (hi < 0.0f || lo >= k.Lx) continue;
                const int ca = lo <= 0.0f ? 0 : vmd_cell_coord(lo, k.inv_cx, k.nxf);
                const int cb = hi >= k.Lx ? k.nxf - 1 : vmd_cell_coord(hi, k.inv_cx, k.nxf);
                const unsigned ja = k.csr[qp * k.nxf + ca], jb = k.csr[qp * k.nxf + cb + 1];
                for (unsigned j = ja; j < jb && !stop; ++j) {
                    const float dx = (xi - k.xr[j]) - sx, dy_ = (yi - k.yr[j]) - sy2, dz_ = (zi - k.zr[j]) - sz2;
                    stop = vmd_within_hit(k.w, vmd_d2(dx, dy_, dz_)) && visit(j, dx, dy_, dz_);
                }
            }
        }
    }
    return stop;
}
// within(): a lane leaves the walk at its first hit
__device__ __forceinline__ bool vmd_within_walk(const vmd_within_walk_t& k, int py, int pz, float xi, float yi, float zi) {
    return vmd_within_walk_each(k, py, pz, xi, yi, zi, [](unsigned, float, float, float) { return true; });
}

// what a lane of a walk in LIST order stands on: entry t of the list c wrapped and binned with vmd_cell_of - the function every cell build
// bins with, on the same fp32 values - so its cell, its pencil (py, pz) and its coordinates are what a build would have stored for it
struct vmd_walk_lane_t { uint32_t cell; int py, pz; float x, y, z; };
__device__ __forceinline__ vmd_walk_lane_t vmd_walk_lane(const vmd_cells_params_t& c, const vmd_within_walk_t& k, int b, int t) {
    vmd_walk_lane_t l;
    l.cell = vmd_cell_of(c, b, t, l.x, l.y, l.z);
    const int pen = (int)(l.cell / (uint32_t)k.nxf);
    l.pz = pen / k.ny; l.py = pen - l.pz * k.ny;
    return l;
}

struct vmd_within_pencil_params_t {
    vmd_within_walk_params_t k;
    const float* stgt; const uint32_t* cs_tgt; int ntgt_pad;
    const float* boxes; int B; vmd_grid_t grid; uint32_t pbc;
    unsigned* count; const uint32_t* skip;
    // FLAGS instantiation: u8[B][ntgt_pad], one byte per SORTED position of the target copy; u32[B][npen + 1], the hits of
    // every pencil (entry npen is not written: the scan's total goes there)
    unsigned char* flags; uint32_t* pen_hits;
};

// The walk with T cell-sorted too: one block (one wave) per (frame, pencil), one lane per target atom of the pencil.
// FLAGS: the same walk also says WHICH sorted entries are in - what k_shell_compact turns into a selection of its own.
template <bool FLAGS>
__global__ __launch_bounds__(64) void k_within_pencil(vmd_within_pencil_params_t p) {
    if (p.skip && *p.skip) return;       // a cell build of this batch overflowed a bucket: the host repeats the batch
    const int lane = threadIdx.x;
    const int b = blockIdx.y, pen = blockIdx.x;
    const vmd_within_walk_t k = vmd_within_walk_setup(p.boxes, b, p.pbc, p.grid, p.k);
    const int pz = pen / k.ny, py = pen - pz * k.ny;
    const uint32_t* cst = p.cs_tgt + (size_t)b * (p.grid.ncell + 1);
    const float* tx = p.stgt + (size_t)b * 3 * p.ntgt_pad;
    const unsigned pbeg = cst[pen * k.nxf], pend = cst[(pen + 1) * k.nxf];
    unsigned total = 0;
    for (unsigned i0 = pbeg; i0 < pend; i0 += VMD_WAVE) {
        const unsigned i = i0 + lane;
        const bool hit = i < pend && vmd_within_walk(k, py, pz, tx[i], tx[p.ntgt_pad + i], tx[2 * (size_t)p.ntgt_pad + i]);
        if (FLAGS) { if (i < pend) p.flags[(size_t)b * p.ntgt_pad + i] = hit ? 1 : 0; }
        total += (unsigned)__popcll(__ballot(hit ? 1 : 0));
    }
    if (FLAGS) { if (lane == 0) p.pen_hits[(size_t)b * (k.ny * k.nz + 1) + pen] = total; }
    if (lane == 0 && total) atomicAdd(&p.count[b], total);
}

// ------------------------------------------------------------------------------------------------ K8: a shell's mask in atom order

struct vmd_within_atoms_params_t {
    vmd_cells_params_t c;       // T as a cell build would read it: raw frame, the GRID's boxes, pbc, index list, grid (pat.m = 0; no outputs)
    vmd_within_walk_params_t k;
    unsigned char* mask; size_t mask_stride;     // u8[B][mask_stride], indexed by ATOM: mask[b][T[t]] = hit
    unsigned* count; const uint32_t* skip;
};

// The walk with T NOT sorted: one lane per list entry t, in list order.  The lane wraps its atom and derives its cell with vmd_cell_of - the
// function every cell build bins with, on the same fp32 values - so an atom on a cell boundary stands in the pencil a build would have put
// it in and sees the neighbour pencils k_within_pencil would have walked for it.  Only R is cell-sorted, so nothing needs a rank: the
// answer goes to mask[b][atom].  Lanes of a wave are spatially unrelated: every lane walks its own windows and the loads do not coalesce;
// with a small R under a large T nearly every lane finds its windows empty and leaves after the cell_start reads.
__global__ __launch_bounds__(256) void k_within_atoms(vmd_within_atoms_params_t p) {
    if (p.skip && *p.skip) return;       // the cell build of R (or another one of this batch) overflowed a bucket: the host repeats the batch
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const vmd_within_walk_t k = vmd_within_walk_setup(p.c.boxes, b, p.c.pbc, p.c.grid, p.k);
    bool hit = false;
    if (t < p.c.nsel) {
        const vmd_walk_lane_t l = vmd_walk_lane(p.c, k, b, t);
        hit = vmd_within_walk(k, l.py, l.pz, l.x, l.y, l.z);
        p.mask[(size_t)b * p.mask_stride + (size_t)vmd_sel_atom(p.c, t)] = hit ? 1 : 0;
    }
    const unsigned long long m = __ballot(hit ? 1 : 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&p.count[b], (unsigned)__popcll(m));
}

// ------------------------------------------------------------------------------------------------ K9: and / or / not over shells

// A shell expression is up to four terms and a truth table.  Every term gets one pass over the target list; pass i ORs h_i << i into the
// atom's byte of bits[b][atom], and k_shell_expr_finish looks the byte up in the table.  live: bit v is set iff h_i can still change the
// outcome of a lane whose byte reads v when the pass starts (the bits of the terms not yet evaluated read 0, so at most 8 of the 16
// values occur).  A lane whose bit is clear does no walk and leaves its byte alone.
struct vmd_within_atoms_expr_params_t {
    vmd_cells_params_t c;       // T as k_within_atoms reads it
    vmd_within_walk_params_t k;
    unsigned char* bits; size_t stride;         // u8[B][stride], indexed by ATOM
    int term; uint32_t live;
    const uint32_t* skip;
};

// The walk of k_within_atoms for ONE term of an expression.  The lane reads its byte first; a wave with no live lane leaves after that one load.
__global__ __launch_bounds__(256) void k_within_atoms_expr(vmd_within_atoms_expr_params_t p) {
    if (p.skip && *p.skip) return;       // a cell build of this batch overflowed a bucket: the host repeats the batch
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    size_t at = 0;
    unsigned cur = 0;
    bool go = false;
    if (t < p.c.nsel) {
        at = (size_t)b * p.stride + (size_t)vmd_sel_atom(p.c, t);
        cur = p.bits[at];
        go = ((p.live >> cur) & 1u) != 0;
    }
    if (!__ballot(go ? 1 : 0)) return;
    const vmd_within_walk_t k = vmd_within_walk_setup(p.c.boxes, b, p.c.pbc, p.c.grid, p.k);
    if (go) {
        const vmd_walk_lane_t l = vmd_walk_lane(p.c, k, b, t);
        if (vmd_within_walk(k, l.py, l.pz, l.x, l.y, l.z)) p.bits[at] = (unsigned char)(cur | (1u << p.term));
    }
}

struct vmd_within_brute_expr_params_t {
    const float* xyz; size_t frame_stride; size_t row_stride;
    const float* boxes; uint32_t pbc; int B;
    const int32_t* tgt; int ntgt; const int32_t* ref; int nref;
    vmd_within_test_t w;
    unsigned char* bits; size_t stride;
    int term; uint32_t live;
    const uint32_t* skip;
};

// The all-pairs twin, for a small R or where no grid exists.  One WAVE per block, so that a wave with no live lane can leave after its one
// load - in front of the first barrier - without leaving a tile half staged.
__global__ __launch_bounds__(64) void k_within_brute_expr(vmd_within_brute_expr_params_t p) {
    __shared__ float s_r[3][256];
    if (p.skip && *p.skip) return;
    const int b = blockIdx.y;
    const int t = blockIdx.x * 64 + threadIdx.x;
    const float* fx = p.xyz + (size_t)b * p.frame_stride;
    const float* fy = fx + p.row_stride;
    const float* fz = fy + p.row_stride;
    size_t at = 0;
    unsigned cur = 0;
    bool go = false;
    int a_t = 0;
    if (t < p.ntgt) {
        a_t = p.tgt ? p.tgt[t] : t;
        at = (size_t)b * p.stride + (size_t)a_t;
        cur = p.bits[at];
        go = ((p.live >> cur) & 1u) != 0;
    }
    if (!__ballot(go ? 1 : 0)) return;
    const vmd_box_t bx = vmd_load_box(p.boxes, b, p.pbc);
    float xi = VMD_FAR, yi = VMD_FAR, zi = VMD_FAR;
    if (go) vmd_pair_coords(bx, fx[a_t], fy[a_t], fz[a_t], xi, yi, zi);
    if (vmd_within_all_pairs<64>(s_r, bx, fx, fy, fz, p.ref, p.nref, p.w, go, xi, yi, zi)) p.bits[at] = (unsigned char)(cur | (1u << p.term));
}

struct vmd_shell_expr_finish_params_t {
    const int32_t* tgt; int ntgt;
    const unsigned char* bits; unsigned char* mask; size_t stride;
    uint32_t truth;
    unsigned* count; const uint32_t* skip;
};

// One lane per entry of T: the byte the term passes left is the index into the truth table (a skipped term reads 0 - the outcome did not
// depend on it).  mask[b][atom] is the layout k_sdf_scatter<.., true> and vmd_eval_shell_mask read; count[b] the population, one atomic per wave.
__global__ __launch_bounds__(256) void k_shell_expr_finish(vmd_shell_expr_finish_params_t p) {
    if (p.skip && *p.skip) return;
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    bool in = false;
    if (t < p.ntgt) {
        const size_t at = (size_t)b * p.stride + (size_t)(p.tgt ? p.tgt[t] : t);
        in = ((p.truth >> p.bits[at]) & 1u) != 0;
        p.mask[at] = in ? 1 : 0;
    }
    const unsigned long long m = __ballot(in ? 1 : 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&p.count[b], (unsigned)__popcll(m));
}

// ------------------------------------------------------------------------------------------------ K7: shells as selections

// Stream compaction of a cell-sorted copy: the entries k_within_pencil<true> flagged, in place order, become a second sorted copy with its
// own cell_start on the SAME grid - a selection k_rdf_pencil takes unchanged.  One wave per (frame, pencil); pen_base is the exclusive
// prefix of the pencils' hit counts (k_cells_scan), so a pencil's output is one contiguous run starting there: a chunk of 64 flags is one
// ballot, an entry's place is the run so far plus the hits below its lane, and a cell's start is the same count taken at the cell's first
// position.  Stable within every cell.  Entries beyond a frame's population keep whatever an earlier batch left there (finite coordinates
// or the zeros of the allocation): k_rdf_pencil reads past a segment only into columns it moves out of every cutoff (x = -VMD_FAR), the same
// terms on which it reads the slack behind a parent's rows.
struct vmd_shell_compact_params_t {
    const unsigned char* flags; const uint32_t* pen_base;
    const float* sorted; const uint32_t* cs; int nsel_pad;
    float* sorted_hit; uint32_t* cs_hit;
    int B; vmd_grid_t grid; const uint32_t* skip;
};

__global__ __launch_bounds__(64) void k_shell_compact(vmd_shell_compact_params_t p) {
    if (p.skip && *p.skip) return;       // the flags were not written either
    const int lane = threadIdx.x;
    const int b = blockIdx.y, pen = blockIdx.x;
    const int nxf = p.grid.nxf, npen = p.grid.ny * p.grid.nz;
    const uint32_t* cs = p.cs + (size_t)b * (p.grid.ncell + 1) + (size_t)pen * nxf;
    uint32_t* csh = p.cs_hit + (size_t)b * (p.grid.ncell + 1) + (size_t)pen * nxf;
    const unsigned char* fl = p.flags + (size_t)b * p.nsel_pad;
    const float* sx = p.sorted + (size_t)b * 3 * p.nsel_pad;
    float* hx = p.sorted_hit + (size_t)b * 3 * p.nsel_pad;
    const unsigned pbeg = cs[0], pend = cs[nxf];
    unsigned run = p.pen_base[(size_t)b * (npen + 1) + pen];
    for (unsigned i0 = pbeg; i0 < pend; i0 += VMD_WAVE) {
        const unsigned i = i0 + lane;
        const bool h = i < pend && fl[i] != 0;
        const unsigned long long m = __ballot(h ? 1 : 0);
        if (h) {
            const unsigned dst = run + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            hx[dst] = sx[i];
            hx[p.nsel_pad + dst] = sx[p.nsel_pad + i];
            hx[2 * (size_t)p.nsel_pad + dst] = sx[2 * (size_t)p.nsel_pad + i];
        }
        for (int c = lane; c < nxf; c += VMD_WAVE) {          // the cells that begin inside this chunk
            const unsigned s = cs[c];
            if (s >= i0 && s < i0 + VMD_WAVE && s < pend) csh[c] = run + (unsigned)__popcll(m & ((1ull << (s - i0)) - 1ull));
        }
        run += (unsigned)__popcll(m);
    }
    for (int c = lane; c < nxf; c += VMD_WAVE) if (cs[c] >= pend) csh[c] = run;       // empty cells at the pencil's end, an empty pencil
    if (pen == npen - 1 && lane == 0) csh[nxf] = run;                                   // cell_start[ncell]: the frame's population
}

__global__ __launch_bounds__(256) void k_within_to_float(const unsigned* count, int B, float* out, const uint32_t* skip) {
    if (skip && *skip) return;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) out[b] = (float)count[b];
}

// ------------------------------------------------------------------------------------------------ K3: SDF alignment (fp64)

// cyclic Jacobi on a symmetric 4x4 — identical operation order to oracle vo_jacobi4
// (VEC = false: the eigenvalues alone - the same rotations of A, V untouched)
template <bool VEC>
__device__ void vmd_jacobi4_t(double A[4][4], double V[4][4]) {
    if (VEC) for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 24; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 3; ++p) for (int q = p + 1; q < 4; ++q) off = off + fabs(A[p][q]);
        if (off == 0.0) break;
        for (int p = 0; p < 3; ++p) {
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double at = fabs(theta);
                double t = 1.0 / (at + sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(t * t + 1.0);
                const double s = t * c;
                for (int k = 0; k < 4; ++k) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 4; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                A[p][q] = 0.0; A[q][p] = 0.0;
                if (VEC) for (int k = 0; k < 4; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
        }
    }
}

__device__ void vmd_jacobi4(double A[4][4], double V[4][4]) { vmd_jacobi4_t<true>(A, V); }

// Horn's symmetric 4x4 matrix of a 3x3 correlation matrix S; its largest eigenvalue belongs to the quaternion of the best rotation
__device__ __forceinline__ void vmd_horn_matrix(const double S[3][3], double N[4][4]) {
    N[0][0] = S[0][0] + S[1][1] + S[2][2];
    N[0][1] = S[1][2] - S[2][1];
    N[0][2] = S[2][0] - S[0][2];
    N[0][3] = S[0][1] - S[1][0];
    N[1][1] = S[0][0] - S[1][1] - S[2][2];
    N[1][2] = S[0][1] + S[1][0];
    N[1][3] = S[2][0] + S[0][2];
    N[2][2] = S[1][1] - S[0][0] - S[2][2];
    N[2][3] = S[1][2] + S[2][1];
    N[3][3] = S[2][2] - S[0][0] - S[1][1];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < i; ++j) N[i][j] = N[j][i];
}

// the rotation of the eigenvector of N for its largest eigenvalue.  Inline form: a kernel that keeps S and R in registers (k_rmsf_rotation)
// calls this one; the column is picked by selects, not by an index into V
__device__ __forceinline__ void vmd_horn_rotation_inline(const double S[3][3], double R[9]) {
    double N[4][4], V[4][4];
    vmd_horn_matrix(S, N);
    vmd_jacobi4_t<true>(N, V);
    double lam = N[0][0], qw = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
#pragma unroll
    for (int i = 1; i < 4; ++i) if (N[i][i] > lam) { lam = N[i][i]; qw = V[0][i]; qx = V[1][i]; qy = V[2][i]; qz = V[3][i]; }
    const double nrm = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    qw = qw / nrm; qx = qx / nrm; qy = qy / nrm; qz = qz / nrm;
    R[0] = 1.0 - 2.0 * (qy * qy + qz * qz);
    R[1] = 2.0 * (qx * qy - qw * qz);
    R[2] = 2.0 * (qx * qz + qw * qy);
    R[3] = 2.0 * (qx * qy + qw * qz);
    R[4] = 1.0 - 2.0 * (qx * qx + qz * qz);
    R[5] = 2.0 * (qy * qz - qw * qx);
    R[6] = 2.0 * (qx * qz - qw * qy);
    R[7] = 2.0 * (qy * qz + qw * qx);
    R[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
}
__device__ void vmd_horn_rotation(const double S[3][3], double R[9]) { vmd_horn_rotation_inline(S, R); }

// a centre of mass in fp64: the weighted sums in the order the atoms are handed over, one division per axis at the end
struct vmd_com_t {
    double sw = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
    __device__ __forceinline__ void add(double w, double x, double y, double z) { sw = sw + w; sx = sx + w * x; sy = sy + w * y; sz = sz + w * z; }
    __device__ __forceinline__ void centre(double& c0, double& c1, double& c2) const { c0 = sx / sw; c1 = sy / sw; c2 = sz / sw; }
};

// walks the unwrap chain of one structure; calls f(a, w, px, py, pz) for every atom in order
template <typename F>
__device__ __forceinline__ void vmd_unwrap_chain(const vmd_frame_t& fr, const int32_t* idx, const float* mass, int m, F f) {
    double qx = 0.0, qy = 0.0, qz = 0.0;
    for (int a = 0; a < m; ++a) {
        const int i = idx[a];
        double x = (double)fr.x[i], y = (double)fr.y[i], z = (double)fr.z[i];
        if (a > 0) {
            double dx = x - qx, dy = y - qy, dz = z - qz;
            vmd_mi3_rint(fr.bx, dx, dy, dz);
            x = qx + dx; y = qy + dy; z = qz + dz;
        }
        qx = x; qy = y; qz = z;
        f(a, mass ? (double)mass[a] : 1.0, x, y, z);
    }
}

// DECISION(D-SDF-UNWRAP) as a switch: with the bonds of the system handed over (vmd_system_t::bonds) a structure is made whole along
// its bond tree - atom order[t] hangs on atom parent[order[t]] (local indices; parent < 0 = the root) - as mdlib's
// md_util_unwrap does (/root/reference/src/viamd.cpp:2257), instead of along the index order.  Positions go to `pos` (m x 3 doubles
// of scratch per thread: a parent is not the atom visited last); the callers then sum in INDEX order, as the chain walk does.
__device__ __forceinline__ void vmd_unwrap_tree(const vmd_frame_t& fr, const int32_t* idx, int m, const int32_t* order, const int32_t* parent,
                                                double* pos) {
    for (int t = 0; t < m; ++t) {
        const int a = order[t], par = parent[a];
        const int i = idx[a];
        double x = (double)fr.x[i], y = (double)fr.y[i], z = (double)fr.z[i];
        if (par >= 0) {
            const double qx = pos[3 * par + 0], qy = pos[3 * par + 1], qz = pos[3 * par + 2];
            double dx = x - qx, dy = y - qy, dz = z - qz;
            vmd_mi3_rint(fr.bx, dx, dy, dz);
            x = qx + dx; y = qy + dy; z = qz + dz;
        }
        pos[3 * a + 0] = x; pos[3 * a + 1] = y; pos[3 * a + 2] = z;
    }
}

struct vmd_align_params_t {
    vmd_frames_t f;
    const int32_t* structs; const float* mass; int K; int m;
    const double* ref_pose;
    float* R32; float* c32; double* M64;
    const int32_t* tree_order; const int32_t* tree_parent;   // [K][m] each, or NULL: unwrap along the index order
    double* tree_pos;                                         // [B*K][m][3] scratch of the tree walk
};

__global__ __launch_bounds__(64) void k_sdf_align(vmd_align_params_t p) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= p.f.B * p.K) return;
    const int b = t / p.K, k = t - b * p.K;
    const vmd_frame_t fr = vmd_frame(p.f, b);
    const int32_t* idx = p.structs + (size_t)k * p.m;
    const float* mass = p.mass ? p.mass + (size_t)k * p.m : nullptr;

    vmd_com_t cm;
    double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    const double* ref = p.ref_pose;
    double com0, com1, com2;
    auto add_com = [&](int, double w, double x, double y, double z) { cm.add(w, x, y, z); };
    auto add_cov = [&](int a, double w, double x, double y, double z) {
        const double c0 = x - com0, c1 = y - com1, c2 = z - com2;
        const double r0 = ref[3 * a + 0], r1 = ref[3 * a + 1], r2 = ref[3 * a + 2];
        const double wc0 = w * c0, wc1 = w * c1, wc2 = w * c2;
        S[0][0] = S[0][0] + wc0 * r0; S[0][1] = S[0][1] + wc0 * r1; S[0][2] = S[0][2] + wc0 * r2;
        S[1][0] = S[1][0] + wc1 * r0; S[1][1] = S[1][1] + wc1 * r1; S[1][2] = S[1][2] + wc1 * r2;
        S[2][0] = S[2][0] + wc2 * r0; S[2][1] = S[2][1] + wc2 * r1; S[2][2] = S[2][2] + wc2 * r2;
    };
    if (p.tree_order) {
        double* pos = p.tree_pos + (size_t)t * 3 * p.m;
        vmd_unwrap_tree(fr, idx, p.m, p.tree_order + (size_t)k * p.m, p.tree_parent + (size_t)k * p.m, pos);
        for (int a = 0; a < p.m; ++a) add_com(a, mass ? (double)mass[a] : 1.0, pos[3 * a + 0], pos[3 * a + 1], pos[3 * a + 2]);
        cm.centre(com0, com1, com2);
        for (int a = 0; a < p.m; ++a) add_cov(a, mass ? (double)mass[a] : 1.0, pos[3 * a + 0], pos[3 * a + 1], pos[3 * a + 2]);
    } else {
        vmd_unwrap_chain(fr, idx, mass, p.m, add_com);
        cm.centre(com0, com1, com2);
        vmd_unwrap_chain(fr, idx, mass, p.m, add_cov);
    }
    double R[9];
    vmd_horn_rotation(S, R);
    float* R32 = p.R32 + (size_t)t * 9;
    float* c32 = p.c32 + (size_t)t * 3;
    for (int i = 0; i < 9; ++i) R32[i] = (float)R[i];
    c32[0] = (float)com0; c32[1] = (float)com1; c32[2] = (float)com2;
    if (p.M64) {
        double* M = p.M64 + (size_t)t * 12;
        for (int r = 0; r < 3; ++r) {
            M[4 * r + 0] = R[3 * r + 0]; M[4 * r + 1] = R[3 * r + 1]; M[4 * r + 2] = R[3 * r + 2];
            M[4 * r + 3] = -(R[3 * r + 0] * com0 + R[3 * r + 1] * com1 + R[3 * r + 2] * com2);
        }
    }
}

__global__ __launch_bounds__(64) void k_sdf_ref_pose(const float* xyz, size_t row_stride, const float* box, uint32_t pbc,
                                                     const int32_t* idx, const float* mass, int m, double* ref_pose,
                                                     const int32_t* tree_order, const int32_t* tree_parent) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const vmd_frame_t fr = vmd_frame(vmd_frames_t{xyz, 0, row_stride, box, pbc, 1}, 0);
    vmd_com_t cm;
    if (tree_order) {
        vmd_unwrap_tree(fr, idx, m, tree_order, tree_parent, ref_pose);      // the pose array doubles as the walk's scratch
        for (int a = 0; a < m; ++a) cm.add(mass ? (double)mass[a] : 1.0, ref_pose[3 * a + 0], ref_pose[3 * a + 1], ref_pose[3 * a + 2]);
    } else {
        vmd_unwrap_chain(fr, idx, mass, m, [&](int a, double w, double x, double y, double z) {
            ref_pose[3 * a + 0] = x; ref_pose[3 * a + 1] = y; ref_pose[3 * a + 2] = z;
            cm.add(w, x, y, z);
        });
    }
    double com0, com1, com2;
    cm.centre(com0, com1, com2);
    for (int a = 0; a < m; ++a) {
        ref_pose[3 * a + 0] = ref_pose[3 * a + 0] - com0;
        ref_pose[3 * a + 1] = ref_pose[3 * a + 1] - com1;
        ref_pose[3 * a + 2] = ref_pose[3 * a + 2] - com2;
    }
}

// Per frame: C = COM of structure 0 and R = max_k |mi(c_k - C)| (padded).  An atom farther than r + R from C is farther than r
// from every c_k (triangle inequality of the minimum-image metric), so the scatter can drop it with ONE test instead of K.
__global__ __launch_bounds__(64) void k_sdf_group(const float* __restrict__ c32, const float* __restrict__ boxes, uint32_t pbc,
                                                  int B, int K, float* __restrict__ group) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const vmd_box_t bx = vmd_load_box(boxes, b, pbc);
    const float* c0 = c32 + (size_t)b * K * 3;
    float r2max = 0.0f;
    for (int k = 1; k < K; ++k) {
        const float* c = c0 + 3 * k;
        float dx = c[0] - c0[0], dy = c[1] - c0[1], dz = c[2] - c0[2];
        vmd_mi3_rintf(bx, dx, dy, dz);
        r2max = fmaxf(r2max, vmd_d2(dx, dy, dz));
    }
    float* g = group + 4 * (size_t)b;
    g[0] = c0[0]; g[1] = c0[1]; g[2] = c0[2];
    g[3] = sqrtf(r2max) * 1.0005f + 1.0e-2f;
}

// ------------------------------------------------------------------------------------------------ K4: SDF scatter

#ifndef VMD_LOAD_NT
#define VMD_LOAD_NT(ptr) __builtin_nontemporal_load(ptr)
#endif
struct vmd_scatter_params_t {
    const float* __restrict__ xyz; size_t frame_stride; size_t row_stride;
    const float* __restrict__ boxes; uint32_t pbc; int B;
    const int32_t* __restrict__ structs; int K; int m;
    const float* __restrict__ R32; const float* __restrict__ c32;
    const int32_t* __restrict__ tgt; const int8_t* __restrict__ owner; int ntgt; float extent; int dim;
    unsigned long long* volume;
    const float* __restrict__ group;   // f32[B][4] from k_sdf_group, or NULL
    int tgt_first, tgt_stride;         // tgt_stride > 0: target t is atom tgt_first + t * tgt_stride (no index list to chase)
    int unowned;                       // 1: no target belongs to any structure (the exclusion rule never applies)
    int nt;                            // 1: the frame is read with non-temporal loads (a pure stream: nothing of it is read twice)
};

// one target atom against structure k of frame b (SPEC S5 scatter).  own_k: structure the atom belongs to (-1 none,
// -2 unknown: search the index list)
__device__ __forceinline__ void vmd_sdf_atom_k(const vmd_scatter_params_t& p, const vmd_box_t& bx, int b, int k, float x, float y, float z,
                                               int own_k, int i) {
    // SPEC D-SDF-EXCL: a target atom is skipped for the structure it belongs to
    if (own_k == k) return;
    if (own_k == -2) {
        const int32_t* sidx = p.structs + (size_t)k * p.m;
        bool own = false;
        for (int a = 0; a < p.m; ++a) own = own || (sidx[a] == i);
        if (own) return;
    }
    const float s = p.extent;
    const float* R = p.R32 + ((size_t)b * p.K + k) * 9;
    const float* c = p.c32 + ((size_t)b * p.K + k) * 3;
    float dx = x - c[0], dy = y - c[1], dz = z - c[2];
    vmd_mi3_rintf(bx, dx, dy, dz);
    const float qx = fmaf(R[2], dz, fmaf(R[1], dy, R[0] * dx));
    const float qy = fmaf(R[5], dz, fmaf(R[4], dy, R[3] * dx));
    const float qz = fmaf(R[8], dz, fmaf(R[7], dy, R[6] * dx));
    const float vscale = (float)p.dim / (2.0f * s);
    const float fdim = (float)p.dim;
    const float tx = (qx + s) * vscale;
    const float ty = (qy + s) * vscale;
    const float tz = (qz + s) * vscale;
    if (tx >= 0.0f && tx < fdim && ty >= 0.0f && ty < fdim && tz >= 0.0f && tz < fdim) {
        const int vx = (int)tx, vy = (int)ty, vz = (int)tz;
        atomicAdd(&p.volume[((size_t)vz * p.dim + vy) * p.dim + vx], 1ull);
    }
}

// group pre-filter (k_sdf_group): can this atom reach ANY structure's cube?  A voxel hit needs |q|_inf < s, hence
// |d| = |q| < sqrt(3) s; with the group sphere (centre g, radius g[3]) one distance test replaces K.
// The argument is the triangle inequality of the minimum-image metric.  Per-axis rounding (orthorhombic) IS that metric;
// rounding in fractional space (triclinic, S5) only agrees with it for vectors shorter than half the smallest cell width, so
// in a triclinic cell the filter is used only while the whole reach stays below that (else every atom goes to the K tests).
__device__ __forceinline__ bool vmd_sdf_near(const vmd_scatter_params_t& p, const vmd_box_t& bx, int b, float x, float y, float z) {
    if (!p.group) return true;
    const float* g = p.group + 4 * (size_t)b;
    const float reach = (1.7320508f * p.extent * 1.0005f + 1.0e-3f) + g[3];
    if (bx.tri) {
        const float ty = bx.yz * bx.iLz, tx1 = bx.xy * bx.iLy, tx2 = (bx.xy * bx.yz - bx.Ly * bx.xz) * (bx.iLy * bx.iLz);
        const float wy = bx.Ly / sqrtf(1.0f + ty * ty), wx = bx.Lx / sqrtf(1.0f + tx1 * tx1 + tx2 * tx2);
        const float wmin = fminf(bx.Lz, fminf(wx, wy));
        if (!(reach < 0.499f * wmin)) return true;
    }
    float dx = x - g[0], dy = y - g[1], dz = z - g[2];
    vmd_mi3_rintf(bx, dx, dy, dz);
    return vmd_d2(dx, dy, dz) <= reach * reach;
}

// Target atoms come in index order, i.e. spatially random: nearly every wave holds a few atoms near the structures, so
// running the K transforms under the divergent mask would cost every wave the full loop at ~5 % lane use.  Instead a block
// first compacts the atoms that pass the group test into LDS (1024 candidates per block, all gathers in flight at once),
// then spreads the (atom, structure) pairs evenly over its threads.
// ARITH: the target list is an arithmetic progression (every water oxygen of a regular solvent box: first + 3 t), so the atom index
// is computed instead of loaded and the coordinate gathers do not wait for an index load - one memory round trip per block
// instead of two (the kernel is bound by the latency of its loads under load: a wave used to live ~12 us).
// ILP atoms per thread: all their gathers are in flight at once.
#define VMD_SDF_CAP 512      // survivors of the group test a block holds in LDS at a time (~1 % of its atoms pass; more take another round)

// The pieces the list kernels share.  The register set of a thread: ILP targets of frame b.
template <int ILP>
struct vmd_sdf_tile_t { int b; int idx[ILP], own[ILP]; float x[ILP], y[ILP], z[ILP]; };

// index and owner of the target slots t0 + STEP * u, then the gathers of all of them (nt: as non-temporal loads)
template <int ILP, bool ARITH, int STEP>
__device__ __forceinline__ void vmd_sdf_targets(const vmd_scatter_params_t& p, int b, int t0, bool nt, vmd_sdf_tile_t<ILP>& T) {
    T.b = b;
    const float* fx = p.xyz + (size_t)b * p.frame_stride;
#pragma unroll
    for (int u = 0; u < ILP; ++u) {
        const int t = t0 + STEP * u;
        T.idx[u] = -1; T.own[u] = p.unowned ? -1 : -2;
        if (t < p.ntgt) {
            T.idx[u] = ARITH ? p.tgt_first + t * p.tgt_stride : (p.tgt ? p.tgt[t] : t);
            if (!p.unowned && p.owner) T.own[u] = (int)p.owner[t];
        }
    }
#pragma unroll
    for (int u = 0; u < ILP; ++u) {
        T.x[u] = T.y[u] = T.z[u] = 0.0f;
        if (T.idx[u] >= 0) {
            if (nt) {
                T.x[u] = VMD_LOAD_NT(fx + T.idx[u]); T.y[u] = VMD_LOAD_NT(fx + p.row_stride + T.idx[u]); T.z[u] = VMD_LOAD_NT(fx + 2 * p.row_stride + T.idx[u]);
            } else {
                T.x[u] = fx[T.idx[u]]; T.y[u] = fx[p.row_stride + T.idx[u]]; T.z[u] = fx[2 * p.row_stride + T.idx[u]];
            }
        }
    }
}

// bit u: target u of the tile passed the group test
template <int ILP>
__device__ __forceinline__ unsigned vmd_sdf_near_mask(const vmd_scatter_params_t& p, const vmd_box_t& bx, const vmd_sdf_tile_t<ILP>& T) {
    unsigned pending = 0u;
#pragma unroll
    for (int u = 0; u < ILP; ++u) if (T.idx[u] >= 0 && vmd_sdf_near(p, bx, T.b, T.x[u], T.y[u], T.z[u])) pending |= 1u << u;
    return pending;
}

// the survivors of one round in LDS: CAP = VMD_SDF_CAP per block, VMD_WAVE per wave
template <int CAP>
struct vmd_sdf_stack_t {
    float x[CAP], y[CAP], z[CAP]; int own[CAP], idx[CAP];
    __device__ __forceinline__ void put(unsigned slot, float px, float py, float pz, int o, int i) {
        x[slot] = px; y[slot] = py; z[slot] = pz; own[slot] = o; idx[slot] = i;
    }
};

// the (survivor, structure) pairs of a stack that holds min(n, CAP) atoms, dealt evenly to nthreads threads
template <int CAP>
__device__ __forceinline__ void vmd_sdf_stack_run(const vmd_scatter_params_t& p, const vmd_box_t& bx, int b, const vmd_sdf_stack_t<CAP>& S,
                                                  unsigned n, int tid, int nthreads) {
    const int nwork = (int)(n < (unsigned)CAP ? n : (unsigned)CAP) * p.K;
    for (int w = tid; w < nwork; w += nthreads) {
        const int a = w / p.K, k = w - a * p.K;
        vmd_sdf_atom_k(p, bx, b, k, S.x[a], S.y[a], S.z[a], S.own[a], S.idx[a]);
    }
}

// per-BLOCK rounds over the NBIT bits of `pending`: every set bit takes a slot (put(bit, slot) fills it from the thread's registers),
// the block runs the stack, and whoever found it full comes back for the next round
template <int NBIT, class PUT>
__device__ __forceinline__ void vmd_sdf_block_rounds(const vmd_scatter_params_t& p, const vmd_box_t& bx, int b, unsigned pending,
                                                     const vmd_sdf_stack_t<VMD_SDF_CAP>& S, unsigned& s_n, PUT put) {
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) s_n = 0u;
        __syncthreads();
#pragma unroll
        for (int bit = 0; bit < NBIT; ++bit) {
            if (pending & (1u << bit)) {
                const unsigned slot = atomicAdd(&s_n, 1u);
                if (slot < VMD_SDF_CAP) { put(bit, slot); pending &= ~(1u << bit); }
            }
        }
        __syncthreads();
        const unsigned total = s_n;
        vmd_sdf_stack_run(p, bx, b, S, total, (int)threadIdx.x, 256);
        if (total <= VMD_SDF_CAP) break;      // block-uniform: everybody read the same s_n
    }
}

// per-WAVE rounds (ballot + prefix, 64 slots): no block barrier
template <int ILP>
__device__ __forceinline__ void vmd_sdf_wave_rounds(const vmd_scatter_params_t& p, const vmd_box_t& bx, const vmd_sdf_tile_t<ILP>& T,
                                                    unsigned pending, int lane, vmd_sdf_stack_t<VMD_WAVE>& S) {
    for (;;) {
        unsigned base = 0u;                                   // wave-uniform: survivors placed in this round
        bool left = false;
#pragma unroll
        for (int u = 0; u < ILP; ++u) {
            const bool hit = (pending >> u) & 1u;
            const unsigned long long m = VMD_BALLOT(hit);
            if (m == 0ull) continue;
            const unsigned pre = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            const unsigned slot = base + pre;
            if (hit && slot < (unsigned)VMD_WAVE) {
                S.put(slot, T.x[u], T.y[u], T.z[u], T.own[u], T.idx[u]);
                pending &= ~(1u << u);
            }
            base += (unsigned)__popcll(m);
            if (base > (unsigned)VMD_WAVE) left = true;
        }
        if (base == 0u) break;
        __builtin_amdgcn_wave_barrier();
        vmd_sdf_stack_run(p, bx, T.b, S, base, lane, VMD_WAVE);
        __builtin_amdgcn_wave_barrier();
        if (!left) break;                                     // wave-uniform
    }
}

// MASKED: the target is a within() shell.  mask is u8[B][mask_stride] indexed by ATOM (k_within_atoms, or k_within_brute<true, true>);
// a target whose byte of frame b is 0 drops out where the group pre-filter drops atoms - everything behind that (D-SDF-EXCL by atom identity,
// the S5 arithmetic, the u64 voxel atomics) is the static path.  The mask hangs on a cell build, so this instantiation alone tests the batch's
// overflow flag, all or nothing: the host launches it where the flag is final and repeats the batch otherwise.
struct vmd_scatter_masked_params_t : vmd_scatter_params_t { const unsigned char* mask; size_t mask_stride; const uint32_t* skip; };
template <bool MASKED> struct vmd_scatter_arg { typedef vmd_scatter_params_t type; };
template <> struct vmd_scatter_arg<true> { typedef vmd_scatter_masked_params_t type; };
template <int ILP, bool ARITH, bool MASKED = false>
__global__ __launch_bounds__(256) void k_sdf_scatter(typename vmd_scatter_arg<MASKED>::type p) {
    if constexpr (MASKED) { if (p.skip && *p.skip) return; }
    __shared__ vmd_sdf_stack_t<VMD_SDF_CAP> S;
    __shared__ unsigned s_n;
    const int b = blockIdx.y;
    const vmd_box_t bx = vmd_load_box(p.boxes, b, p.pbc);
    vmd_sdf_tile_t<ILP> T;
    vmd_sdf_targets<ILP, ARITH, 256>(p, b, blockIdx.x * (256 * ILP) + threadIdx.x, p.nt != 0, T);
    if constexpr (MASKED) {
        const unsigned char* mk = p.mask + (size_t)b * p.mask_stride;
#pragma unroll
        for (int u = 0; u < ILP; ++u) if (T.idx[u] >= 0 && mk[T.idx[u]] == 0) T.idx[u] = -1;
    }
    vmd_sdf_block_rounds<ILP>(p, bx, b, vmd_sdf_near_mask<ILP>(p, bx, T), S, s_n,
                              [&](int u, unsigned slot) { S.put(slot, T.x[u], T.y[u], T.z[u], T.own[u], T.idx[u]); });
}

// Wave-level variant (A/B, `sdf_wave`): the survivors of the group test are compacted per WAVE (ballot + prefix, 64 slots of LDS per
// wave and round) instead of per block, so the kernel has no block barrier at all - a wave that found nothing near the structures
// (most of them: ~1 % of the atoms pass) retires as soon as its loads are tested.
template <int ILP, bool ARITH>
__global__ __launch_bounds__(256) void k_sdf_scatter_wave(vmd_scatter_params_t p) {
    __shared__ vmd_sdf_stack_t<VMD_WAVE> S[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.y;
    const vmd_box_t bx = vmd_load_box(p.boxes, b, p.pbc);
    vmd_sdf_tile_t<ILP> T;
    vmd_sdf_targets<ILP, ARITH, VMD_WAVE>(p, b, blockIdx.x * (256 * ILP) + wave * (VMD_WAVE * ILP) + lane, false, T);      // a wave owns 64 * ILP consecutive targets
    vmd_sdf_wave_rounds<ILP>(p, bx, T, vmd_sdf_near_mask<ILP>(p, bx, T), lane, S[wave]);
}

// Streaming variant (`sdf_wave` = 2): the one-shot kernels above retire a block after ~12 KB of gathers and pay the launch of its
// successor (kernel arguments, box and group record, index arithmetic - about a microsecond in which the wave slot has nothing in
// flight) once per 1 024 atoms.  Here the grid is persistent: a wave walks the (frame, 64 * ILP targets) tiles w, w + W, w + 2 W, ...
// (consecutive waves on consecutive tiles, so the grid reads one moving window of the trajectory) and issues the gathers of its NEXT
// tile before it tests the current one - two register sets, the wave always has a tile in flight.  Survivors of the group test
// are compacted per wave as in k_sdf_scatter_wave (no block barrier).  Same arithmetic, same result.
template <int ILP, bool ARITH>
__device__ __forceinline__ void vmd_sdf_tile_load(const vmd_scatter_params_t& p, long long tile, int tiles_per_frame, int lane, vmd_sdf_tile_t<ILP>& T) {
    const int b = (int)(tile / tiles_per_frame);
    const int c = (int)(tile - (long long)b * tiles_per_frame);
    vmd_sdf_targets<ILP, ARITH, VMD_WAVE>(p, b, c * (VMD_WAVE * ILP) + lane, false, T);
}

template <int ILP>
__device__ __forceinline__ void vmd_sdf_tile_scatter(const vmd_scatter_params_t& p, const vmd_sdf_tile_t<ILP>& T, int lane, vmd_sdf_stack_t<VMD_WAVE>& S) {
    const vmd_box_t bx = vmd_load_box(p.boxes, T.b, p.pbc);
    const unsigned pending = vmd_sdf_near_mask<ILP>(p, bx, T);
    if (VMD_BALLOT(pending != 0u) == 0ull) return;          // ~99 % of the atoms fail the group test: most tiles end here
    vmd_sdf_wave_rounds<ILP>(p, bx, T, pending, lane, S);
}

template <int ILP, bool ARITH>
__global__ __launch_bounds__(256) void k_sdf_scatter_stream(vmd_scatter_params_t p, int tiles_per_frame) {
    __shared__ vmd_sdf_stack_t<VMD_WAVE> S[4];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const long long W = (long long)gridDim.x * 4;
    const long long ntiles = (long long)tiles_per_frame * p.B;
    long long tile = (long long)blockIdx.x * 4 + wave;
    if (tile >= ntiles) return;
    vmd_sdf_tile_t<ILP> A, B2;
    vmd_sdf_tile_load<ILP, ARITH>(p, tile, tiles_per_frame, lane, A);
    for (;;) {
        const bool more1 = tile + W < ntiles;                 // wave-uniform
        if (more1) vmd_sdf_tile_load<ILP, ARITH>(p, tile + W, tiles_per_frame, lane, B2);
        vmd_sdf_tile_scatter<ILP>(p, A, lane, S[wave]);
        if (!more1) break;
        tile += W;
        const bool more2 = tile + W < ntiles;
        if (more2) vmd_sdf_tile_load<ILP, ARITH>(p, tile + W, tiles_per_frame, lane, A);
        vmd_sdf_tile_scatter<ILP>(p, B2, lane, S[wave]);
        if (!more2) break;
        tile += W;
    }
}

// Row-streaming variant for arithmetic-progression targets (first + t * stride, e.g. every water oxygen: stride 3): the lines of
// the x / y / z rows are needed in full anyway (a stride-3 selection touches every 32-byte sector), so a thread takes GPT groups of
// 4 consecutive ATOMS with 16-byte loads - three perfectly coalesced dwordx4 loads per group instead of twelve strided dword
// gathers - and tests only the atoms of its groups that are targets (one or two of four for stride 3).  Survivors of the group
// test go through the same bounded LDS compaction and K-structure loop as in k_sdf_scatter; same arithmetic, same result.
template <int GPT>
__global__ __launch_bounds__(256) void k_sdf_scatter_rows(vmd_scatter_params_t p, int g_first, int ngroups) {
    __shared__ vmd_sdf_stack_t<VMD_SDF_CAP> S;
    __shared__ unsigned s_n;
    const int b = blockIdx.y;
    const vmd_box_t bx = vmd_load_box(p.boxes, b, p.pbc);
    const float* fx = p.xyz + (size_t)b * p.frame_stride;
    const int s = p.tgt_stride, first = p.tgt_first;
    vmd_f4a x4[GPT], y4[GPT], z4[GPT];
    int a0[GPT];
#pragma unroll
    for (int u = 0; u < GPT; ++u) {
        const int gl = (blockIdx.x * GPT + u) * 256 + threadIdx.x;
        a0[u] = -1;
        if (gl < ngroups) {
            a0[u] = 4 * (g_first + gl);
            x4[u] = *(const vmd_f4a*)(fx + a0[u]);
            y4[u] = *(const vmd_f4a*)(fx + p.row_stride + a0[u]);
            z4[u] = *(const vmd_f4a*)(fx + 2 * p.row_stride + a0[u]);
        }
    }
    unsigned pending = 0u;          // bit 4u + k: atom k of group u is a target that passed the group test
#pragma unroll
    for (int u = 0; u < GPT; ++u) {
        if (a0[u] < 0) continue;
        // first target at or after atom a0: offset k0 in [0, s)
        const int d = a0[u] - first;
        int k0 = d >= 0 ? (s - d % s) % s : -d;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k != k0) continue;
            const int t = (a0[u] + k - first) / s;
            if (t < p.ntgt && vmd_sdf_near(p, bx, b, x4[u][k], y4[u][k], z4[u][k])) pending |= 1u << (4 * u + k);
            k0 += s;
        }
    }
    vmd_sdf_block_rounds<4 * GPT>(p, bx, b, pending, S, s_n, [&](int bit, unsigned slot) {
        const int u = bit >> 2, k = bit & 3, idx = a0[u] + k;
        S.put(slot, x4[u][k], y4[u][k], z4[u][k], p.unowned ? -1 : (p.owner ? (int)p.owner[(idx - first) / s] : -2), idx);
    });
}

// dense targets (a sizeable fraction of all atoms, e.g. every water oxygen): stream the WHOLE frame with 16-byte loads per
// lane and pick the targets by a per-atom tag byte (255 = not a target, 254 = target, k <= 253 = target owned by structure k)
// instead of gathering 4 bytes per lane through an index list.  Same arithmetic, same result.
__global__ __launch_bounds__(256) void k_sdf_scatter_dense(vmd_scatter_params_t p, const uint8_t* __restrict__ tag, int natoms4) {
    const int t4 = blockIdx.x * 256 + threadIdx.x;       // group of 4 consecutive atoms
    const int b = blockIdx.y;
    if (t4 >= natoms4) return;
    const uint32_t tg = ((const uint32_t*)tag)[t4];
    if (tg == 0xffffffffu) return;
    const vmd_box_t bx = vmd_load_box(p.boxes, b, p.pbc);
    const float* fx = p.xyz + (size_t)b * p.frame_stride;
    const vmd_f4a x4 = *(const vmd_f4a*)(fx + 4 * (size_t)t4);
    const vmd_f4a y4 = *(const vmd_f4a*)(fx + p.row_stride + 4 * (size_t)t4);
    const vmd_f4a z4 = *(const vmd_f4a*)(fx + 2 * p.row_stride + 4 * (size_t)t4);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int tu = (int)((tg >> (8 * u)) & 255u);
        if (tu == 255 || !vmd_sdf_near(p, bx, b, x4[u], y4[u], z4[u])) continue;
        for (int k = 0; k < p.K; ++k) vmd_sdf_atom_k(p, bx, b, k, x4[u], y4[u], z4[u], tu == 254 ? -1 : tu, 4 * t4 + u);
    }
}

// ------------------------------------------------------------------------------------------------ K5: distances

struct vmd_dist_params_t {
    vmd_frames_t f;
    // population of P contexts (`... in residue(:)`): context c uses a[aoff[c]..aoff[c+1]) and b[boff[c]..boff[c+1])
    const int32_t* a; const float* mass_a; const int32_t* aoff; const int32_t* b; const float* mass_b; const int32_t* boff; int P;
    int per;      // values per context: 1, or |a_c|*|b_c| for distance_pair (equal for all contexts)
    float* out;   // [B][P*per]
};

__device__ void vmd_set_com(const vmd_frame_t& fr,const int32_t* idx, const float* mass, int n, float out[3]) {
    vmd_com_t cm;
    double p0x = 0.0, p0y = 0.0, p0z = 0.0;
    for (int a = 0; a < n; ++a) {
        const int i = idx[a];
        double x = (double)fr.x[i], y = (double)fr.y[i], z = (double)fr.z[i];
        if (a == 0) { p0x = x; p0y = y; p0z = z; }
        else {
            double dx = x - p0x, dy = y - p0y, dz = z - p0z;
            vmd_mi3_rint(fr.bx, dx, dy, dz);
            x = p0x + dx; y = p0y + dy; z = p0z + dz;
        }
        cm.add(mass ? (double)mass[a] : 1.0, x, y, z);
    }
    double c0, c1, c2;
    cm.centre(c0, c1, c2);
    out[0] = (float)c0; out[1] = (float)c1; out[2] = (float)c2;
}

__global__ __launch_bounds__(64) void k_distance_com(vmd_dist_params_t p) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= p.f.B * p.P) return;
    const int b = t / p.P, c = t - b * p.P;
    const vmd_frame_t fr = vmd_frame(p.f, b);
    const int a0 = p.aoff[c], na = p.aoff[c + 1] - a0, b0 = p.boff[c], nb = p.boff[c + 1] - b0;
    float ca[3], cb[3];
    vmd_set_com(fr, p.a + a0, p.mass_a ? p.mass_a + a0 : nullptr, na, ca);
    vmd_set_com(fr, p.b + b0, p.mass_b ? p.mass_b + b0 : nullptr, nb, cb);
    float dx = ca[0] - cb[0], dy = ca[1] - cb[1], dz = ca[2] - cb[2];
    vmd_mi3_rintf(fr.bx, dx, dy, dz);
    p.out[t] = sqrtf(vmd_d2(dx, dy, dz));
}

__device__ __forceinline__ float vmd_pair_d2(const vmd_frame_t& fr, int i, int j) {
    float xi, yi, zi, xj, yj, zj;
    vmd_pair_coords(fr.bx, fr.x[i], fr.y[i], fr.z[i], xi, yi, zi);
    vmd_pair_coords(fr.bx, fr.x[j], fr.y[j], fr.z[j], xj, yj, zj);
    return vmd_pair_d2_general(fr.bx, xi, yi, zi, xj, yj, zj);
}

// one block per (frame, context); MAXI = false -> min, true -> max
template <bool MAXI>
__global__ __launch_bounds__(256) void k_distance_minmax(vmd_dist_params_t p) {
    __shared__ float s_red[256];
    const int b = blockIdx.x / p.P, c = blockIdx.x - b * p.P;
    const int a0 = p.aoff[c], na = p.aoff[c + 1] - a0, b0 = p.boff[c], nb = p.boff[c + 1] - b0;
    const long long npairs = (long long)na * nb;
    const vmd_frame_t fr = vmd_frame(p.f, b);
    float best = MAXI ? 0.0f : 3.4028235e38f;
    for (long long k = threadIdx.x; k < npairs; k += 256) {
        const int ia = (int)(k / nb), ib = (int)(k - (long long)ia * nb);
        const float d2 = vmd_pair_d2(fr, p.a[a0 + ia], p.b[b0 + ib]);
        best = MAXI ? fmaxf(best, d2) : fminf(best, d2);
    }
    s_red[threadIdx.x] = best;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const float v = s_red[threadIdx.x + o];
            s_red[threadIdx.x] = MAXI ? fmaxf(s_red[threadIdx.x], v) : fminf(s_red[threadIdx.x], v);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) p.out[blockIdx.x] = sqrtf(s_red[0]);
}

// grid (B*P, ceil(per/256)): all |a_c| x |b_c| pairs of context c, row-major.  The (frame, context) index sits on grid.x: a
// population of >= 64 contexts over a 1 024-frame batch exceeds the 65 535 limit of grid.y
__global__ __launch_bounds__(256) void k_distance_pair(vmd_dist_params_t p) {
    const long long k = (long long)blockIdx.y * 256 + threadIdx.x;
    const int b = blockIdx.x / p.P, c = blockIdx.x - b * p.P;
    if (k >= p.per) return;
    const int a0 = p.aoff[c], b0 = p.boff[c], nb = p.boff[c + 1] - b0;
    const int ia = (int)(k / nb), ib = (int)(k - (long long)ia * nb);
    p.out[((size_t)b * p.P + c) * p.per + k] = sqrtf(vmd_pair_d2(vmd_frame(p.f, b), p.a[a0 + ia], p.b[b0 + ib]));
}

// ------------------------------------------------------------------------------------------------ K5b: angle / dihedral (DESIGN S6b)

struct vmd_geom_params_t {
    vmd_frames_t f;
    // argument k of context c: set[k][off[k][c] .. off[k][c+1]), masses parallel to set[k]
    const int32_t* set[4]; const float* mass[4]; const int32_t* off[4]; int P;
    int radians;  // D-ANGLE-UNIT: 0 = degrees
    float* out;   // [B][P]
};

// a x b, components in the order DESIGN S6b writes them
__device__ __forceinline__ void vmd_cross_d(double ax, double ay, double az, double bx, double by, double bz, double& cx, double& cy,
                                            double& cz) {
    cx = ay * bz - az * by;
    cy = az * bx - ax * bz;
    cz = ax * by - ay * bx;
}
__device__ __forceinline__ double vmd_dot_d(double ax, double ay, double az, double bx, double by, double bz) {
    return (ax * bx + ay * by) + az * bz;
}

// fp32 minimum-image bond vector q - p of two points
__device__ __forceinline__ void vmd_bond(const vmd_box_t& bx, const float p[3], const float q[3], float d[3]) {
    d[0] = q[0] - p[0]; d[1] = q[1] - p[1]; d[2] = q[2] - p[2];
    vmd_mi3_rintf(bx, d[0], d[1], d[2]);
}
__device__ __forceinline__ void vmd_normal(const float a[3], const float b[3], double n[3]) {
    vmd_cross_d(a[0], a[1], a[2], b[0], b[1], b[2], n[0], n[1], n[2]);
}
// the dihedral, in radians (IUPAC sign), from its first two bond vectors and the two normals n1 = b1 x b2, n2 = b2 x b3.  `+ 0.0` turns a
// -0 operand of atan2 into +0: degenerate input gives atan2(+0, +0) = 0 (D-ANGLE-DEGENERATE) and a dihedral never comes out as -180.
__device__ __forceinline__ double vmd_dihedral(const float b1[3], const float b2[3], const double n1[3], const double n2[3]) {
    const double l2 = sqrt(vmd_dot_d(b2[0], b2[1], b2[2], b2[0], b2[1], b2[2]));
    const double y = l2 * vmd_dot_d(b1[0], b1[1], b1[2], n2[0], n2[1], n2[2]);
    return atan2(y + 0.0, vmd_dot_d(n1[0], n1[1], n1[2], n2[0], n2[1], n2[2]) + 0.0);
}

// one thread per (frame, context): the NARG argument points are the S6 centres of distance(a, b) (vmd_set_com), joined by fp32
// minimum-image differences (vmd_bond); the value is formed in fp64 (no contraction) and rounded once.
template <int NARG>
__global__ __launch_bounds__(64) void k_geom(vmd_geom_params_t p) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= p.f.B * p.P) return;
    const int b = t / p.P, c = t - b * p.P;
    const vmd_frame_t fr = vmd_frame(p.f, b);
    float q[NARG][3];
#pragma unroll
    for (int k = 0; k < NARG; ++k) {
        const int k0 = p.off[k][c], n = p.off[k][c + 1] - k0;
        vmd_set_com(fr, p.set[k] + k0, p.mass[k] + k0, n, q[k]);
    }
    double rad;
    if constexpr (NARG == 3) {
        // angle(a, b, c) at the middle point: u = mi(pa - pb), v = mi(pc - pb)
        float u[3], v[3];
        double n[3];
        vmd_bond(fr.bx, q[1], q[0], u);
        vmd_bond(fr.bx, q[1], q[2], v);
        vmd_normal(u, v, n);
        const double s = sqrt(vmd_dot_d(n[0], n[1], n[2], n[0], n[1], n[2]));
        rad = atan2(s + 0.0, vmd_dot_d(u[0], u[1], u[2], v[0], v[1], v[2]) + 0.0);
    } else {
        // dihedral(a, b, c, d): b1 = mi(pb - pa), b2 = mi(pc - pb), b3 = mi(pd - pc)
        float d[3][3];
        double n1[3], n2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) vmd_bond(fr.bx, q[k], q[k + 1], d[k]);
        vmd_normal(d[0], d[1], n1);
        vmd_normal(d[1], d[2], n2);
        rad = vmd_dihedral(d[0], d[1], n1, n2);
    }
    p.out[t] = p.radians ? (float)rad : (float)(rad * (180.0 / M_PI));
}

// ------------------------------------------------------------------------------------------------ K10: backbone phi / psi, Ramachandran map

struct vmd_bb_params_t {
    vmd_frames_t f;
    const int32_t* n; const int32_t* ca; const int32_t* c; const uint8_t* link; int nseg;
    float* out;   // [B][nseg][2]
};

typedef float vmd_f2a __attribute__((vector_size(8)));     // {phi, psi}: one 8-byte access (the table's rows are 8-byte aligned)

// one thread per (frame, segment), the segment fastest: five gathers, four bond vectors, three normals (the one of N-CA-C serves both
// angles), two atan2, one 8-byte store.  A single-atom set of k_geom is the atom's raw position (vmd_set_com: w x / w is exact) and both
// kernels call vmd_bond / vmd_dihedral, so phi and psi are dihedral()'s values bit for bit.  DECISION(D-BB-ENDS): the angle that lacks its
// neighbour is +0.
__global__ __launch_bounds__(64) void k_backbone_angles(vmd_bb_params_t p) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= p.f.B * p.nseg) return;
    const int b = t / p.nseg, s = t - b * p.nseg;
    const vmd_frame_t fr = vmd_frame(p.f, b);
    const unsigned lk = p.link[s];
    const bool prev = (lk & 1u) && s > 0, next = (lk & 2u) && s + 1 < p.nseg;
    const int in = p.n[s], ia = p.ca[s], ic = p.c[s];
    const float N[3] = {fr.x[in], fr.y[in], fr.z[in]}, A[3] = {fr.x[ia], fr.y[ia], fr.z[ia]}, C[3] = {fr.x[ic], fr.y[ic], fr.z[ic]};
    float b1[3], b2[3];
    vmd_bond(fr.bx, N, A, b1);
    vmd_bond(fr.bx, A, C, b2);
    double nm[3];
    vmd_normal(b1, b2, nm);
    float phi = 0.0f, psi = 0.0f;
    if (prev) {
        const int ip = p.c[s - 1];
        const float Cp[3] = {fr.x[ip], fr.y[ip], fr.z[ip]};
        float b0[3];
        double n0[3];
        vmd_bond(fr.bx, Cp, N, b0);
        vmd_normal(b0, b1, n0);
        phi = (float)vmd_dihedral(b0, b1, n0, nm);
    }
    if (next) {
        const int iq = p.n[s + 1];
        const float Nn[3] = {fr.x[iq], fr.y[iq], fr.z[iq]};
        float b3[3];
        double n3[3];
        vmd_bond(fr.bx, C, Nn, b3);
        vmd_normal(b2, b3, n3);
        psi = (float)vmd_dihedral(b1, b2, nm, n3);
    }
    vmd_f2a o;
    o[0] = phi; o[1] = psi;
    *(vmd_f2a*)(p.out + 2 * (size_t)t) = o;
}

struct vmd_rama_params_t {
    const float* angles; int F; int nseg;
    const uint8_t* row_mask; const uint8_t* rama_class; const uint8_t* link; int skip_ends;
    unsigned long long* counts; unsigned long long* sums;
};

// DECISION(D-RAMA-BIN): the reference's fp32 expression, every operation rounded on its own (this file is compiled without contraction);
// u lies in [0, 1], and u = 1 (phi = fl32(pi)) wraps to column 0
__device__ __forceinline__ unsigned vmd_rama_coord(float a) {
    const float scale = (float)(1.0 / (2.0 * M_PI));
    const float u = (a * scale) + 0.5f;
    return (unsigned)(u * (float)VMD_RAMA_DIM) & (unsigned)(VMD_RAMA_DIM - 1);
}

// one thread per table entry: one no-return 64-bit atomic per binned sample, the class sums through a ballot per class (one atomic per
// wave and class).  No lane leaves before the ballots.
__global__ __launch_bounds__(256) void k_rama_bin(vmd_rama_params_t p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = t < (long long)p.F * p.nseg;
    int cls = -1;
    unsigned x = 0, y = 0;
    if (live) {
        const int r = (int)(t / p.nseg), s = (int)(t - (long long)r * p.nseg);
        const unsigned c = p.rama_class[s];
        bool go = c < (unsigned)VMD_RAMA_CLASSES && (!p.row_mask || p.row_mask[r] != 0);
        if (go && p.skip_ends) go = (p.link[s] & 3u) == 3u;
        if (go) {
            const vmd_f2a a = *(const vmd_f2a*)(p.angles + 2 * (size_t)t);
            if (!(a[0] == 0.0f && a[1] == 0.0f)) { cls = (int)c; x = vmd_rama_coord(a[0]); y = vmd_rama_coord(a[1]); }
        }
    }
    if (cls >= 0) atomicAdd(&p.counts[((size_t)y * VMD_RAMA_DIM + x) * VMD_RAMA_CLASSES + (unsigned)cls], 1ull);
    if (!p.sums) return;
    for (int c = 0; c < VMD_RAMA_CLASSES; ++c) {
        const unsigned long long m = __ballot(cls == c ? 1 : 0);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&p.sums[c], (unsigned long long)__popcll(m));
    }
}

// ------------------------------------------------------------------------------------------------ K11: secondary structure

// Four bit matrices per frame, rows of W = ceil(nseg / 64) 64-bit words: HB[a] bit d and HBT[d] bit a = hb(a, d) (the C=O of a accepts from
// the N-H of d), BP[i] bit j / BA[i] bit j = parallel / antiparallel bridge (i, j).  Bits at and above nseg are zero in every row.
struct vmd_ss_params_t {
    vmd_frames_t f;
    const int32_t* n; const int32_t* ca; const int32_t* c; const int32_t* o;
    const int32_t* rng;                 // [nseg] the range of every segment
    const uint8_t* pro;                 // [nseg] 1 = proline
    const unsigned long long* nbmask;   // [W] bit j: j has both neighbours in its range
    int nseg; int W;
    unsigned long long* hb; unsigned long long* hbt; unsigned long long* bp; unsigned long long* ba;     // [B][nseg][W] each
    float* cls;                         // [B][nseg]
    float* pop;                         // [B][VMD_SS_CODES]
};

__device__ __forceinline__ int vmd_imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int vmd_imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ double vmd_ss_len(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

// D-SS-HBOND for a gated pair: ON / CN are the fp32 minimum-image vectors N[d] - O[a] and N[d] - C[a], u the donor's unit C=O direction
__device__ __forceinline__ bool vmd_ss_bond(const float on[3], const float cn[3], const double u[3]) {
    const double rON = vmd_ss_len((double)on[0], (double)on[1], (double)on[2]);
    const double rCN = vmd_ss_len((double)cn[0], (double)cn[1], (double)cn[2]);
    const double rOH = vmd_ss_len((double)on[0] + u[0], (double)on[1] + u[1], (double)on[2] + u[2]);
    const double rCH = vmd_ss_len((double)cn[0] + u[0], (double)cn[1] + u[1], (double)cn[2] + u[2]);
    if (rON < 0.5 || rCN < 0.5 || rOH < 0.5 || rCH < 0.5) return true;
    return 27.888 * (((1.0 / rON + 1.0 / rCH) - 1.0 / rOH) - 1.0 / rCN) < -0.5;
}

// one wave per (frame, word of 64 donors, word of 64 acceptors): the donors live in the lanes (their N, CA and unit C=O vector are made once),
// the 64 acceptors are staged in LDS and walked one at a time.  Only the CA gate is tested in that walk: a pair that passes is pushed on
// the wave's LDS stack, and whenever 64 pairs stand there they take a lane each for the energy - the gate passes for a few lanes per
// acceptor, and fp64 square roots and divisions on four lanes of 64 were four fifths of this kernel.  A bond sets its bit in the two
// 64 x 64 bit blocks in LDS; at the end every lane stores one word of HB (acceptor wa * 64 + lane, donors w) and one of HBT.
__global__ __launch_bounds__(64) void k_ss_hbond(vmd_ss_params_t p) {
    __shared__ float s_pos[64][9];      // CA, C, O of the acceptors
    __shared__ int s_rng[64];
    __shared__ int s_acc[64];           // the acceptor has an oxygen
    __shared__ float s_n[64][3];        // the donors' N ...
    __shared__ double s_u[64][3];       // ... and unit C=O vector
    __shared__ unsigned short s_stack[128];      // gated pairs: donor lane << 6 | acceptor
    __shared__ unsigned s_hb[64][2], s_hbt[64][2];      // [acceptor] bits by donor lane, [donor lane] bits by acceptor, two halves each
    const int lane = threadIdx.x;
    const long long blk = blockIdx.x;
    const int w = (int)(blk % p.W), wa = (int)((blk / p.W) % p.W), b = (int)(blk / ((long long)p.W * p.W));
    const vmd_frame_t fr = vmd_frame(p.f, b);
    const int al = wa * 64 + lane;
    s_acc[lane] = 0; s_rng[lane] = -1;
    s_hb[lane][0] = s_hb[lane][1] = s_hbt[lane][0] = s_hbt[lane][1] = 0u;
    if (al < p.nseg) {
        const int ia = p.ca[al], ic = p.c[al], io = p.o[al];
        s_pos[lane][0] = fr.x[ia]; s_pos[lane][1] = fr.y[ia]; s_pos[lane][2] = fr.z[ia];
        s_pos[lane][3] = fr.x[ic]; s_pos[lane][4] = fr.y[ic]; s_pos[lane][5] = fr.z[ic];
        if (io >= 0) { s_pos[lane][6] = fr.x[io]; s_pos[lane][7] = fr.y[io]; s_pos[lane][8] = fr.z[io]; s_acc[lane] = 1; }
        s_rng[lane] = p.rng[al];
    }
    const int d = w * 64 + lane;
    bool donor = false;
    int rd = -2;
    float A[3] = {0.0f, 0.0f, 0.0f};
    if (d < p.nseg) {
        rd = p.rng[d];
        const int ia = p.ca[d];
        A[0] = fr.x[ia]; A[1] = fr.y[ia]; A[2] = fr.z[ia];
        // D-SS-H: the amide H sits at N[d] + u, u the unit vector of mi(C[d-1] - O[d-1])
        if (d > 0 && p.rng[d - 1] == rd && !p.pro[d] && p.o[d - 1] >= 0) {
            const int ic = p.c[d - 1], io = p.o[d - 1], in = p.n[d];
            float v[3] = {fr.x[ic] - fr.x[io], fr.y[ic] - fr.y[io], fr.z[ic] - fr.z[io]};
            vmd_mi3_rintf(fr.bx, v[0], v[1], v[2]);
            const double l = vmd_ss_len((double)v[0], (double)v[1], (double)v[2]);
            if (l > 0.0) {
                donor = true;
                s_u[lane][0] = (double)v[0] / l; s_u[lane][1] = (double)v[1] / l; s_u[lane][2] = (double)v[2] / l;
                s_n[lane][0] = fr.x[in]; s_n[lane][1] = fr.y[in]; s_n[lane][2] = fr.z[in];
            }
        }
    }
    __syncthreads();
    // the energy of stack entry e, by whichever lane holds it
    auto bond = [&](unsigned e) {
        const int dl = (int)(e >> 6), j = (int)(e & 63u);
        float on[3] = {s_n[dl][0] - s_pos[j][6], s_n[dl][1] - s_pos[j][7], s_n[dl][2] - s_pos[j][8]};
        float cn[3] = {s_n[dl][0] - s_pos[j][3], s_n[dl][1] - s_pos[j][4], s_n[dl][2] - s_pos[j][5]};
        vmd_mi3_rintf(fr.bx, on[0], on[1], on[2]);
        vmd_mi3_rintf(fr.bx, cn[0], cn[1], cn[2]);
        const double u[3] = {s_u[dl][0], s_u[dl][1], s_u[dl][2]};
        if (vmd_ss_bond(on, cn, u)) {
            atomicOr(&s_hb[j][dl >> 5], 1u << (dl & 31));
            atomicOr(&s_hbt[dl][j >> 5], 1u << (j & 31));
        }
    };
    const int na = vmd_imin(64, p.nseg - wa * 64);
    unsigned top = 0u;                  // entries on the stack (the same in every lane)
    for (int j = 0; j < na; ++j) {
        const int a = wa * 64 + j;
        bool gate = false;
        if (donor && s_acc[j] && a != d && !(d == a + 1 && s_rng[j] == rd)) {
            float g[3] = {A[0] - s_pos[j][0], A[1] - s_pos[j][1], A[2] - s_pos[j][2]};
            vmd_mi3_rintf(fr.bx, g[0], g[1], g[2]);
            gate = ((double)g[0] * (double)g[0] + (double)g[1] * (double)g[1]) + (double)g[2] * (double)g[2] < 81.0;
        }
        const unsigned long long m = __ballot(gate ? 1 : 0);
        if (gate) s_stack[top + (unsigned)__popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)((lane << 6) | j);
        top += (unsigned)__popcll(m);
        if (top >= 64u) {               // < 64 before the push, < 128 after it: the top 64 entries take a lane each
            __syncthreads();
            top -= 64u;
            bond(s_stack[top + lane]);
            __syncthreads();
        }
    }
    __syncthreads();
    if ((unsigned)lane < top) bond(s_stack[lane]);
    __syncthreads();
    if (al < p.nseg) p.hb[((size_t)b * p.nseg + al) * p.W + w] = (unsigned long long)s_hb[lane][0] | ((unsigned long long)s_hb[lane][1] << 32);
    if (d < p.nseg) p.hbt[((size_t)b * p.nseg + d) * p.W + wa] = (unsigned long long)s_hbt[lane][0] | ((unsigned long long)s_hbt[lane][1] << 32);
}

// word w of a bit row moved by one bit, with the carry of the neighbouring word: bit j of the result is bit j + 1 (down) / j - 1 (up) of the row
__device__ __forceinline__ unsigned long long vmd_ss_down(const unsigned long long* row, int w, int W) {
    return (row[w] >> 1) | (w + 1 < W ? row[w + 1] << 63 : 0ull);
}
__device__ __forceinline__ unsigned long long vmd_ss_up(const unsigned long long* row, int w) {
    return (row[w] << 1) | (w > 0 ? row[w - 1] >> 63 : 0ull);
}

// one thread per (frame, segment i, word): the four bridge patterns of DESIGN 1.12 (5) as ANDs of rows of HB / HBT and of their one-bit
// moves, masked with "j has both neighbours" and, inside i's range, |i - j| >= 3.  A row whose i lacks a neighbour is zero.
__global__ __launch_bounds__(256) void k_ss_bridges(vmd_ss_params_t p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)p.f.B * p.nseg * p.W) return;
    const int w = (int)(t % p.W), i = (int)((t / p.W) % p.nseg);
    const size_t b = (size_t)(t / ((long long)p.W * p.nseg));
    unsigned long long par = 0ull, anti = 0ull;
    if (i >= 1 && i + 1 < p.nseg && p.rng[i - 1] == p.rng[i] && p.rng[i + 1] == p.rng[i]) {
        const unsigned long long* hb = p.hb + (b * p.nseg + i) * p.W;       // row i; rows i - 1 and i + 1 stand W words before and behind
        const unsigned long long* hbt = p.hbt + (b * p.nseg + i) * p.W;
        anti = (hb[w] & hbt[w]) | (vmd_ss_down(hb - p.W, w, p.W) & vmd_ss_up(hbt + p.W, w));
        par = ((hb - p.W)[w] & (hbt + p.W)[w]) | (vmd_ss_up(hbt, w) & vmd_ss_down(hb, w, p.W));
        unsigned long long keep = p.nbmask[w];
        for (int j = vmd_imax(i - 2, 0); j <= vmd_imin(i + 2, p.nseg - 1); ++j)
            if ((j >> 6) == w && p.rng[j] == p.rng[i]) keep &= ~(1ull << (j & 63));
        par &= keep; anti &= keep;
    }
    p.bp[t] = par;
    p.ba[t] = anti;
}

// one block per frame, the seven passes of DESIGN 1.12 (7) with a barrier between them; the codes of a pass stand in one LDS row while the
// next pass writes the other.  Pass 1 takes a wave per segment (lanes over the words of its rows, one ballot each for "has a bridge" and
// "is in a ladder"); the later passes take a thread per segment.  The populations: one ballot per code and wave, summed in the wave's
// registers, one LDS atomic per wave and code at the end.
__global__ __launch_bounds__(256) void k_ss_assign(vmd_ss_params_t p) {
    HIP_DYNAMIC_SHARED(uint32_t, s_dyn)             // three rows of nseg bytes (rounded up to 16), at most 3 x VMD_SS_SEG_MAX = 48 KB
    __shared__ unsigned s_pop[VMD_SS_CODES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.x;
    const int nseg = p.nseg, W = p.W;
    uint8_t* s_turn = (uint8_t*)s_dyn;              // bit 0 / 1 / 2: turn_3 / turn_4 / turn_5 starts here
    uint8_t* s_c0 = s_turn + ((nseg + 15) & ~15);
    uint8_t* s_c1 = s_c0 + ((nseg + 15) & ~15);
    const unsigned long long* HB = p.hb + b * nseg * W;
    const unsigned long long* BP = p.bp + b * nseg * W;
    const unsigned long long* BA = p.ba + b * nseg * W;
    if (tid < VMD_SS_CODES) s_pop[tid] = 0u;
    // pass 1: bridge / sheet; the turn bits
    for (int i = wave; i < nseg; i += 4) {
        bool bridge = false, ladder = false;
        for (int w0 = 0; w0 < W; w0 += 64) {
            const int w = w0 + lane;
            if (w < W) {
                const unsigned long long* bp = BP + (size_t)i * W;
                const unsigned long long* ba = BA + (size_t)i * W;
                bridge = bridge || (bp[w] | ba[w]) != 0ull;
                unsigned long long pn = 0ull, an = 0ull;       // partners (j) whose neighbour continues the ladder
                if (i + 1 < nseg) { pn |= vmd_ss_down(bp + W, w, W); an |= vmd_ss_up(ba + W, w); }
                if (i > 0) { pn |= vmd_ss_up(bp - W, w); an |= vmd_ss_down(ba - W, w, W); }
                ladder = ladder || ((bp[w] & pn) | (ba[w] & an)) != 0ull;
            }
        }
        const unsigned long long mb = __ballot(bridge ? 1 : 0), ml = __ballot(ladder ? 1 : 0);
        if (lane == 0) {
            s_c0[i] = ml ? 8 : (mb ? 7 : 0);
            unsigned tb = 0u;
            for (int n = 3; n <= 5; ++n) {
                const int j = i + n;
                if (j < nseg && p.rng[j] == p.rng[i] && ((HB[(size_t)i * W + (j >> 6)] >> (j & 63)) & 1ull)) tb |= 1u << (n - 3);
            }
            s_turn[i] = (uint8_t)tb;
        }
    }
    __syncthreads();
    // pass 2: two consecutive 4-turns write an alpha helix over anything
    for (int i = tid; i < nseg; i += 256) {
        bool hx = false;
        for (int s = vmd_imax(i - 3, 1); s <= i; ++s) hx = hx || ((s_turn[s - 1] & 2u) && (s_turn[s] & 2u));
        s_c1[i] = hx ? 5 : s_c0[i];
    }
    __syncthreads();
    // pass 3: two consecutive 3-turns, three unassigned segments
    for (int i = tid; i < nseg; i += 256) {
        bool hx = false;
        for (int s = vmd_imax(i - 2, 1); s <= i; ++s)
            hx = hx || ((s_turn[s - 1] & 1u) && (s_turn[s] & 1u) && s_c1[s] == 0 && s_c1[s + 1] == 0 && s_c1[s + 2] == 0);
        s_c0[i] = hx ? 4 : s_c1[i];
    }
    __syncthreads();
    // pass 4: two consecutive 5-turns, five unassigned segments
    for (int i = tid; i < nseg; i += 256) {
        bool hx = false;
        for (int s = vmd_imax(i - 4, 1); s <= i; ++s)
            hx = hx || ((s_turn[s - 1] & 4u) && (s_turn[s] & 4u) && s_c0[s] == 0 && s_c0[s + 1] == 0 && s_c0[s + 2] == 0 && s_c0[s + 3] == 0
                        && s_c0[s + 4] == 0);
        s_c1[i] = hx ? 6 : s_c0[i];
    }
    __syncthreads();
    // passes 5 - 7: turn, bend, coil; the class row and the populations
    const vmd_frame_t fr = vmd_frame(p.f, (int)b);
    unsigned cnt[VMD_SS_CODES];
#pragma unroll
    for (int k = 0; k < VMD_SS_CODES; ++k) cnt[k] = 0u;
    for (int i0 = 0; i0 < nseg; i0 += 256) {
        const int i = i0 + tid;
        int code = -1;
        if (i < nseg) {
            code = s_c1[i];
            if (code == 0) {
                bool turn = false;
                for (int n = 3; n <= 5; ++n)
                    for (int k = 1; k < n; ++k) turn = turn || (i - k >= 0 && (s_turn[i - k] & (1u << (n - 3))));
                code = turn ? 2 : 1;
                if (!turn && i >= 2 && i + 2 < nseg && p.rng[i - 2] == p.rng[i] && p.rng[i + 2] == p.rng[i]) {
                    const int i0a = p.ca[i - 2], i1a = p.ca[i], i2a = p.ca[i + 2];
                    const float A0[3] = {fr.x[i0a], fr.y[i0a], fr.z[i0a]}, A1[3] = {fr.x[i1a], fr.y[i1a], fr.z[i1a]};
                    const float A2[3] = {fr.x[i2a], fr.y[i2a], fr.z[i2a]};
                    float a[3], c[3];
                    vmd_bond(fr.bx, A0, A1, a);
                    vmd_bond(fr.bx, A1, A2, c);
                    const double aa = vmd_dot_d(a[0], a[1], a[2], a[0], a[1], a[2]), cc = vmd_dot_d(c[0], c[1], c[2], c[0], c[1], c[2]);
                    const double q = aa * cc;
                    if (q > 0.0 && vmd_dot_d(a[0], a[1], a[2], c[0], c[1], c[2]) / sqrt(q) < 0.3420201433256687) code = 3;
                }
            }
            p.cls[b * nseg + i] = (float)code;
        }
#pragma unroll
        for (int k = 1; k < VMD_SS_CODES; ++k) cnt[k] += (unsigned)__popcll(__ballot(code == k ? 1 : 0));
    }
    if (lane == 0)
        for (int k = 1; k < VMD_SS_CODES; ++k) if (cnt[k]) atomicAdd(&s_pop[k], cnt[k]);
    __syncthreads();
    if (tid < VMD_SS_CODES) p.pop[b * VMD_SS_CODES + tid] = (float)s_pop[tid];
}

// ------------------------------------------------------------------------------------------------ K5c: shape_weights

// ---- the set reduction of K5c and K5d (rules 1 - 5): its order is a function of the set size alone.  (1) A set is cut into
// chunks of VMD_SET_CHUNK atoms, atom j of a chunk belongs to thread j % VMD_SET_BLOCK; (2) a thread adds its atoms in increasing j;
// (3) the 64 lanes of a wave are summed by the xor butterfly 32, 16, 8, 4, 2, 1 (vmd_set_wave_sum); (4) the four waves of the block as
// ((w0 + w1) + w2) + w3 (vmd_set_block_sum); (5) the chunks in increasing order (vmd_set_chunk_sum).  None of the helpers owns LDS.
#define VMD_SET_CHUNK 4096
#define VMD_SET_BLOCK 256
#define VMD_SET_STEPS (VMD_SET_CHUNK / VMD_SET_BLOCK)       // atoms per thread and chunk
#define VMD_SET_WAVES (VMD_SET_BLOCK / 64)
#define VMD_SET_WAVE_SET 64        // a population whose largest set has at most this many atoms: one wave per set (the _small kernels)
#define VMD_RMSD_GROUP 2           // atoms a thread takes per step of k_rmsd_moments (loads first, one barrier per step); the others take 4
static_assert(VMD_SET_STEPS == 16, "rule 2 and the pinned restatements of the tests: at most 16 atoms per thread and chunk");
static_assert(VMD_SET_STEPS % 4 == 0 && VMD_SET_STEPS % VMD_RMSD_GROUP == 0, "a step's atoms divide the chunk's steps");
static_assert(VMD_SET_WAVES == 4, "rule 4 is written out for four waves");
static_assert(VMD_SET_WAVE_SET == 64, "a _small kernel holds one atom per lane");

__host__ __device__ inline int vmd_set_chunks(int n) { return (n + VMD_SET_CHUNK - 1) / VMD_SET_CHUNK; }

// context c of a population: its atoms are set[k0 .. k0 + n), masses parallel to them
struct vmd_set_slice_t { int k0, n; };
__device__ __forceinline__ vmd_set_slice_t vmd_set_slice(const int32_t* off, int c) {
    const int k0 = off[c];
    return vmd_set_slice_t{k0, off[c + 1] - k0};
}
// block blockIdx.x of a (frame, context, chunk) grid: bc = b * P + c, a0 = the chunk's first atom.  False: the whole block leaves (a context
// with fewer chunks than the largest set).
struct vmd_set_block_t { int chunk, bc, b, c, a0; vmd_set_slice_t s; };
__device__ __forceinline__ bool vmd_set_block(const int32_t* off, int P, int nchunk, vmd_set_block_t& w) {
    w.chunk = blockIdx.x % nchunk; w.bc = blockIdx.x / nchunk;
    w.b = w.bc / P; w.c = w.bc - w.b * P;
    w.s = vmd_set_slice(off, w.c);
    w.a0 = w.chunk * VMD_SET_CHUNK;
    return w.a0 < w.s.n;
}

// both 32-bit halves of a double through the float shuffle (bit moves)
__device__ __forceinline__ double vmd_shfl_xor_f64(double v, int o) {
    int h[2];
    __builtin_memcpy(h, &v, 8);
    h[0] = __float_as_int(__shfl_xor(__int_as_float(h[0]), o));
    h[1] = __float_as_int(__shfl_xor(__int_as_float(h[1]), o));
    __builtin_memcpy(&v, h, 8);
    return v;
}
template <int N>
__device__ __forceinline__ void vmd_set_wave_sum(double s[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[k] = s[k] + vmd_shfl_xor_f64(s[k], o);
}
// the block's N sums from its waves' (every lane of a wave holds the wave's), through the caller's s_wave: out[k] by thread k
template <class T, int N>
__device__ __forceinline__ void vmd_set_block_sum(const T s[N], T (*s_wave)[N], T* out) {
    const int tid = threadIdx.x;
    if ((tid & 63) == 0)
#pragma unroll
        for (int k = 0; k < N; ++k) s_wave[tid >> 6][k] = s[k];
    __syncthreads();
    if (tid < N) out[tid] = ((s_wave[0][tid] + s_wave[1][tid]) + s_wave[2][tid]) + s_wave[3][tid];
}
// the sums of a set of n atoms from its chunks' partials q[chunk][N]
template <int N>
__device__ __forceinline__ void vmd_set_chunk_sum(const double* q, int n, double s[N]) {
    const int nch = vmd_set_chunks(n);
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = q[k];
    for (int ch = 1; ch < nch; ++ch)
#pragma unroll
        for (int k = 0; k < N; ++k) s[k] = s[k] + q[ch * N + k];
}
// what rules 4 and 5 make of a wave's sum when the set is one wave of one chunk: three empty waves add +0 (a -0 becomes +0)
__device__ __forceinline__ double vmd_set_small_sum(double v) { return ((v + 0.0) + 0.0) + 0.0; }

// A frame's cell in fp64 with 1 / L, once per thread.  Orthorhombic axes avoid the division in the common case: d - L rint(d / L) needs only
// the INTEGER nearest to d / L, and q = d * (1 / L) is within 2^-51 |q| of the quotient, so rint(q) is that integer unless q lies that
// close to a half-integer (vmd_set_round_sure); then (and for huge |q|) the quotient itself is formed - one rare branch per atom, behind
// the loads.
struct vmd_set_frame_t { vmd_frame_t fr; double Lx, Ly, Lz, iLx, iLy, iLz, xy, xz, yz; };
__device__ __forceinline__ vmd_set_frame_t vmd_set_frame(const vmd_frames_t& f, int b) {
    vmd_set_frame_t s;
    s.fr = vmd_frame(f, b);
    s.Lx = (double)s.fr.bx.Lx; s.Ly = (double)s.fr.bx.Ly; s.Lz = (double)s.fr.bx.Lz;
    s.xy = (double)s.fr.bx.xy; s.xz = (double)s.fr.bx.xz; s.yz = (double)s.fr.bx.yz;
    s.iLx = 1.0 / s.Lx; s.iLy = 1.0 / s.Ly; s.iLz = 1.0 / s.Lz;
    return s;
}
__device__ __forceinline__ bool vmd_set_round_sure(double q, double r) { return fabs(q - r) < 0.499999 && fabs(q) < 1.0e9; }

// Atom a of the set in two steps, so that a thread has the loads of several atoms in flight before it looks at the first (a branch
// between two loads makes the compiler wait for each of them).  An atom past the end is read as atom 0 with weight 0: every term is
// +-0 and leaves the sums as they are.
struct vmd_set_atom_t { float x, y, z, w; };
__device__ __forceinline__ vmd_set_atom_t vmd_set_load(const vmd_frame_t& fr, const int32_t* set, const float* mass, int a, int n) {
    const bool live = a < n;
    const int aa = live ? a : 0;
    const int i = set[aa];
    vmd_set_atom_t q;
    q.x = fr.x[i]; q.y = fr.y[i]; q.z = fr.z[i];
    const float m = mass[aa];
    q.w = live ? m : 0.0f;
    return q;
}

struct vmd_shape_params_t {
    vmd_frames_t f;
    const int32_t* set; const float* mass; const int32_t* off; int P;   // context c: set[off[c] .. off[c+1]), masses parallel to set
    int nchunk;        // chunks of the largest set
    double* partial;   // [B][P][nchunk][10]: W, S1 x y z, S2 xx xy xz yy yz zz
    float* lin; float* plan; float* iso;   // [B][P] each
};

// The shape kernels' offset e = mi(x - x_first), vmd_mi3_rint bit for bit
__device__ __forceinline__ void vmd_shape_mi(const vmd_set_frame_t& s, double& dx, double& dy, double& dz) {
    const vmd_box_t& bx = s.fr.bx;
    if (bx.tri) { vmd_mi3_rint(bx, dx, dy, dz); return; }
    const double qx = dx * s.iLx, qy = dy * s.iLy, qz = dz * s.iLz;
    double rx = rint(qx), ry = rint(qy), rz = rint(qz);
    const bool sure = (!bx.px || vmd_set_round_sure(qx, rx)) && (!bx.py || vmd_set_round_sure(qy, ry)) && (!bx.pz || vmd_set_round_sure(qz, rz));
    if (__builtin_expect(!sure, 0)) { rx = rint(dx / s.Lx); ry = rint(dy / s.Ly); rz = rint(dz / s.Lz); }
    if (bx.px) dx = dx - s.Lx * rx;
    if (bx.py) dy = dy - s.Ly * ry;
    if (bx.pz) dz = dz - s.Lz * rz;
}

// the ten moments of one atom added to s
__device__ __forceinline__ void vmd_shape_add(const vmd_set_atom_t& q, const vmd_set_frame_t& bx, double p0x, double p0y, double p0z,
                                              double s[10]) {
    const double w = (double)q.w;
    double ex = (double)q.x - p0x, ey = (double)q.y - p0y, ez = (double)q.z - p0z;
    vmd_shape_mi(bx, ex, ey, ez);
    const double wx = w * ex, wy = w * ey, wz = w * ez;
    s[0] = s[0] + w;
    s[1] = s[1] + wx; s[2] = s[2] + wy; s[3] = s[3] + wz;
    s[4] = s[4] + wx * ex; s[5] = s[5] + wx * ey; s[6] = s[6] + wx * ez;
    s[7] = s[7] + wy * ey; s[8] = s[8] + wy * ez; s[9] = s[9] + wz * ez;
}

// Westin's measures of M = S2 - S1 S1^T / W: eigenvalues by cyclic Jacobi (pairs (0,1), (0,2), (1,2), at most 16 sweeps, ends when the
// off-diagonal is exactly 0), sorted, clamped at 0.  t == 0 or W == 0: 0, 0, 0 (D-SHAPE-DEGENERATE).
__device__ void vmd_shape_values(const double s[10], float& lin, float& plan, float& iso) {
    lin = 0.0f; plan = 0.0f; iso = 0.0f;
    const double W = s[0];
    if (W == 0.0) return;
    double a00 = s[4] - (s[1] * s[1]) / W, a01 = s[5] - (s[1] * s[2]) / W, a02 = s[6] - (s[1] * s[3]) / W;
    double a11 = s[7] - (s[2] * s[2]) / W, a12 = s[8] - (s[2] * s[3]) / W, a22 = s[9] - (s[3] * s[3]) / W;
    for (int sweep = 0; sweep < 16; ++sweep) {
        if ((fabs(a01) + fabs(a02)) + fabs(a12) == 0.0) break;
#pragma unroll
        for (int pair = 0; pair < 3; ++pair) {
            // (p, q, r): the rotated pair and the third index
            double& app = pair == 2 ? a11 : a00;
            double& aqq = pair == 0 ? a11 : a22;
            double& apq = pair == 0 ? a01 : (pair == 1 ? a02 : a12);
            double& arp = pair == 0 ? a02 : (pair == 1 ? a01 : a01);     // A[r][p]
            double& arq = pair == 0 ? a12 : (pair == 1 ? a12 : a02);     // A[r][q]
            if (apq == 0.0) continue;
            const double theta = (aqq - app) / (2.0 * apq);
            double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
            if (theta < 0.0) t = -t;
            const double c = 1.0 / sqrt(t * t + 1.0);
            const double sn = t * c;
            const double rp = arp, rq = arq;
            arp = c * rp - sn * rq;
            arq = sn * rp + c * rq;
            app = app - t * apq;
            aqq = aqq + t * apq;
            apq = 0.0;
        }
    }
    double l1 = a00, l2 = a11, l3 = a22, h;
    if (l1 < l2) { h = l1; l1 = l2; l2 = h; }
    if (l2 < l3) { h = l2; l2 = l3; l3 = h; }
    if (l1 < l2) { h = l1; l1 = l2; l2 = h; }
    l1 = l1 < 0.0 ? 0.0 : l1; l2 = l2 < 0.0 ? 0.0 : l2; l3 = l3 < 0.0 ? 0.0 : l3;
    const double t = (l1 + l2) + l3;
    if (t == 0.0) return;
    lin = (float)((l1 - l2) / t);
    plan = (float)((2.0 * (l2 - l3)) / t);
    iso = (float)((3.0 * l3) / t);
}

// one block per (frame, context, chunk): ten fp64 sums per thread in registers, wave butterfly, the four wave sums through LDS
__global__ __launch_bounds__(VMD_SET_BLOCK) void k_shape_moments(vmd_shape_params_t p) {
    __shared__ double s_wave[VMD_SET_WAVES][10];
    vmd_set_block_t w;
    if (!vmd_set_block(p.off, p.P, p.nchunk, w)) return;
    const vmd_set_frame_t sf = vmd_set_frame(p.f, w.b);
    const int32_t* set = p.set + w.s.k0;
    const float* mass = p.mass + w.s.k0;
    const int i0 = set[0];
    const double p0x = (double)sf.fr.x[i0], p0y = (double)sf.fr.y[i0], p0z = (double)sf.fr.z[i0];
    double s[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int tid = threadIdx.x;
    // four atoms per step: their sixteen loads first, then the sums in atom order
#pragma unroll 1
    for (int k = 0; k < VMD_SET_STEPS; k += 4) {
        vmd_set_atom_t q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = vmd_set_load(sf.fr, set, mass, w.a0 + (k + u) * VMD_SET_BLOCK + tid, w.s.n);
#pragma unroll
        for (int u = 0; u < 4; ++u) vmd_shape_add(q[u], sf, p0x, p0y, p0z, s);
    }
    vmd_set_wave_sum<10>(s);
    vmd_set_block_sum<double, 10>(s, s_wave, p.partial + (size_t)blockIdx.x * 10);
}

// one thread per (frame, context): the chunk sums in chunk order, then the three values
__global__ __launch_bounds__(64) void k_shape_finish(vmd_shape_params_t p) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= p.f.B * p.P) return;
    double s[10];
    vmd_set_chunk_sum<10>(p.partial + (size_t)t * p.nchunk * 10, vmd_set_slice(p.off, t % p.P).n, s);
    vmd_shape_values(s, p.lin[t], p.plan[t], p.iso[t]);
}

// populations of small sets (`... in residue(:)`): one wave per (frame, context), lane j holds atom j; the same sums in the same order as
// k_shape_moments + k_shape_finish give for such a set (one chunk, one atom per thread, three empty waves), without the partials
__global__ __launch_bounds__(VMD_SET_BLOCK) void k_shape_small(vmd_shape_params_t p) {
    const int t = blockIdx.x * VMD_SET_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= p.f.B * p.P) return;   // the whole wave
    const int b = t / p.P, c = t - b * p.P;
    const vmd_set_slice_t sl = vmd_set_slice(p.off, c);
    const vmd_set_frame_t sf = vmd_set_frame(p.f, b);
    const int32_t* set = p.set + sl.k0;
    const int i0 = set[0];
    const double p0x = (double)sf.fr.x[i0], p0y = (double)sf.fr.y[i0], p0z = (double)sf.fr.z[i0];
    double s[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    vmd_shape_add(vmd_set_load(sf.fr, set, p.mass + sl.k0, lane, sl.n), sf, p0x, p0y, p0z, s);
    vmd_set_wave_sum<10>(s);
    if (lane != 0) return;
#pragma unroll
    for (int k = 0; k < 10; ++k) s[k] = vmd_set_small_sum(s[k]);
    vmd_shape_values(s, p.lin[t], p.plan[t], p.iso[t]);
}

// ------------------------------------------------------------------------------------------------ K5d: rmsd

// `name = rmsd(sel)`: the mass-weighted RMSD of a set after the best rigid fit onto its own pose at trajectory frame 0.  The set is made
// whole along its index chain with INTEGER link shifts (n_a = -rint(frac(x_a - x_{a-1})), k_a = n_1 + ... + n_a: a prefix sum any order
// of which gives the same result), the offsets e_a = (x_a - x_0) + cart(k_a) enter thirteen fp64 sums, and Horn's largest eigenvalue
// gives the value without the rotation.  The reduction is shape_weights' (the vmd_set_* helpers of K5c).
#define VMD_RMSD_NSUM 14           // S1 x y z, G, C xx xy xz yx yy yz zx zy zz (C_ij = sum (w e_i) u_j), W (the pose pass only)
#define VMD_RMSD_NCONST 8          // the pose's constants per context: W, U1 x y z, Gu (three unused)

struct vmd_rmsd_params_t {
    vmd_frames_t f;
    const int32_t* set; const float* mass; const int32_t* off; int P;   // context c: set[off[c] .. off[c+1]), masses parallel to set
    int nchunk;         // chunks of the largest set
    int32_t* shift;     // [B][P][nchunk][4]: the chunk's total link shift x y z (one unused)
    double* partial;    // [B][P][nchunk][VMD_RMSD_NSUM]
    double* pose;       // [off[P]][3]: u_a, parallel to set (written by the pose pass, read by the frame pass)
    double* cst;        // [P][VMD_RMSD_NCONST]
    int zero_row;       // the row of this batch that is trajectory frame 0 (its value is +0 by definition), or -1
    float* out;         // [B][P]
};

// -rint(d / L) as an integer, 0 on an axis that is open.  Only the integer is needed, so the quotient is formed through 1 / L unless that
// could round to the other side of a half-integer (vmd_set_round_sure); then the division itself decides.  An axis flagged periodic
// whose length is not > 0 counts as open HERE and not in vmd_set_frame: the evaluator clears such flags itself (batch_pbc) but the C ABI
// can be called with them set, the integer of d / 0 is undefined, and shape_weights (vmd_shape_mi) keeps what its division gives.
__device__ __forceinline__ int vmd_rmsd_axis_shift(bool periodic, double d, double L, double iL) {
    if (!(periodic && L > 0.0)) return 0;
    const double q = d * iL;
    double r = rint(q);
    if (__builtin_expect(!vmd_set_round_sure(q, r), 0)) r = rint(d / L);
    return -(int)r;
}
// the lattice vector k in Cartesian components, in this written-out order
__device__ __forceinline__ void vmd_rmsd_cart(const vmd_set_frame_t& b, int kx, int ky, int kz, double& cx, double& cy, double& cz) {
    const double fx = (double)kx, fy = (double)ky, fz = (double)kz;
    if (b.fr.bx.tri) {
        cx = (fx * b.Lx + b.xy * fy) + b.xz * fz;
        cy = fy * b.Ly + b.yz * fz;
        cz = fz * b.Lz;
    } else { cx = fx * b.Lx; cy = fy * b.Ly; cz = fz * b.Lz; }
}

// Atom a of the set and its predecessor in the chain, loaded together (all loads of a step stand before its first branch, as in
// k_shape_moments).  An atom past the end is read as atom 0 with weight 0; atom 0 is its own predecessor: both have link shift 0.
struct vmd_rmsd_atom_t { vmd_set_atom_t at; float qx, qy, qz; };
__device__ __forceinline__ vmd_rmsd_atom_t vmd_rmsd_load(const vmd_frame_t& fr, const int32_t* set, const float* mass, int a, int n) {
    vmd_rmsd_atom_t q;
    const int j = set[a < n && a > 0 ? a - 1 : 0];      // both index loads in front of the coordinates' (k_rmsd_shift: 64 VGPRs, 73 the other way)
    q.at = vmd_set_load(fr, set, mass, a, n);
    q.qx = fr.x[j]; q.qy = fr.y[j]; q.qz = fr.z[j];
    return q;
}
__device__ __forceinline__ void vmd_rmsd_link(const vmd_rmsd_atom_t& q, const vmd_set_frame_t& b, int& nx, int& ny, int& nz) {
    const double dx = (double)q.at.x - (double)q.qx, dy = (double)q.at.y - (double)q.qy, dz = (double)q.at.z - (double)q.qz;
    if (b.fr.bx.tri) {
        const double sz = dz / b.Lz;
        const double sy = (dy - b.yz * sz) / b.Ly;
        const double sx = ((dx - b.xy * sy) - b.xz * sz) / b.Lx;
        nx = -(int)rint(sx); ny = -(int)rint(sy); nz = -(int)rint(sz);
        return;
    }
    nx = vmd_rmsd_axis_shift(b.fr.bx.px, dx, b.Lx, b.iLx);
    ny = vmd_rmsd_axis_shift(b.fr.bx.py, dy, b.Ly, b.iLy);
    nz = vmd_rmsd_axis_shift(b.fr.bx.pz, dz, b.Lz, b.iLz);
}

__device__ __forceinline__ int vmd_shfl_xor_i32(int v, int o) { return __float_as_int(__shfl_xor(__int_as_float(v), o)); }
// inclusive prefix sum over the 64 lanes of a wave and the wave's total, by the xor butterfly (integers: the order does not matter)
__device__ __forceinline__ void vmd_wave_scan_i32(int v, int lane, int& incl, int& total) {
    incl = v; total = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = vmd_shfl_xor_i32(total, o);
        if (lane & o) incl += t;
        total += t;
    }
}

// the link shift of one atom scanned over its wave: incl = the shifts of the lanes up to and including this one, tot = the wave's.  A
// molecule that is whole in the cell has no shift along most of its chain: a wave without any skips its three scans
__device__ __forceinline__ void vmd_rmsd_wave_shift(const vmd_rmsd_atom_t& q, const vmd_set_frame_t& b, int lane, int incl[3], int tot[3]) {
    int nx, ny, nz;
    vmd_rmsd_link(q, b, nx, ny, nz);
    if (__ballot((nx | ny | nz) != 0) == 0ull) { incl[0] = incl[1] = incl[2] = tot[0] = tot[1] = tot[2] = 0; return; }
    vmd_wave_scan_i32(nx, lane, incl[0], tot[0]);
    vmd_wave_scan_i32(ny, lane, incl[1], tot[1]);
    vmd_wave_scan_i32(nz, lane, incl[2], tot[2]);
}
// one step's wave totals joined: k = the shift of this thread's atom (what ran in front of the step, the waves in front of its own, its
// own scan); run advances by the whole step
__device__ __forceinline__ void vmd_rmsd_join(const int (*tot)[3], int wave, const int incl[3], int run[3], int k[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) k[i] = run[i] + incl[i];
#pragma unroll
    for (int v = 0; v < VMD_SET_WAVES; ++v)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int t = tot[v][i];
            if (v < wave) k[i] += t;
            run[i] += t;
        }
}
// e_a = (x_a - x_0) + cart(k_a)
__device__ __forceinline__ void vmd_rmsd_offset(const vmd_set_atom_t& q, const vmd_set_frame_t& b, double x0, double y0, double z0,
                                                int kx, int ky, int kz, double& ex, double& ey, double& ez) {
    double cx, cy, cz;
    vmd_rmsd_cart(b, kx, ky, kz, cx, cy, cz);
    ex = ((double)q.x - x0) + cx; ey = ((double)q.y - y0) + cy; ez = ((double)q.z - z0) + cz;
}

// the sums of one atom: k = its accumulated shift, u = its pose offset (frame pass) / where its pose offset goes (pose pass, live atoms)
template <bool POSE>
__device__ __forceinline__ void vmd_rmsd_add(const vmd_set_atom_t& q, const vmd_set_frame_t& b, double x0, double y0, double z0,
                                             int kx, int ky, int kz, const double u[3], double* pose_out, double s[VMD_RMSD_NSUM]) {
    const double w = (double)q.w;
    double ex, ey, ez;
    vmd_rmsd_offset(q, b, x0, y0, z0, kx, ky, kz, ex, ey, ez);
    const double wx = w * ex, wy = w * ey, wz = w * ez;
    s[0] = s[0] + wx; s[1] = s[1] + wy; s[2] = s[2] + wz;
    s[3] = s[3] + ((wx * ex + wy * ey) + wz * ez);
    if (POSE) {
        s[13] = s[13] + w;
        if (pose_out) { pose_out[0] = ex; pose_out[1] = ey; pose_out[2] = ez; }
    } else {
        s[4] = s[4] + wx * u[0]; s[5] = s[5] + wx * u[1]; s[6] = s[6] + wx * u[2];
        s[7] = s[7] + wy * u[0]; s[8] = s[8] + wy * u[1]; s[9] = s[9] + wy * u[2];
        s[10] = s[10] + wz * u[0]; s[11] = s[11] + wz * u[1]; s[12] = s[12] + wz * u[2];
    }
}

// S_ij = C_ij - (S1_i U1_j) / W of the finish, from the sums and the pose's constants
__device__ __forceinline__ void vmd_rmsd_corr(const double s[VMD_RMSD_NSUM], const double* cst, double S[3][3]) {
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) S[i][j] = s[4 + 3 * i + j] - (s[i] * cst[1 + j]) / cst[0];
}

// the value from the thirteen sums and the pose's constants: Horn's largest eigenvalue, no rotation matrix
__device__ float vmd_rmsd_value(const double s[VMD_RMSD_NSUM], const double* cst, int n) {
    const double W = cst[0];
    if (n <= 1 || W == 0.0) return 0.0f;                    // D-RMSD-DEGENERATE
    const double U1[3] = {cst[1], cst[2], cst[3]}, Gu = cst[4];
    const double Gp = s[3] - ((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]) / W;
    const double Gq = Gu - ((U1[0] * U1[0] + U1[1] * U1[1]) + U1[2] * U1[2]) / W;
    double S[3][3], N[4][4];
    vmd_rmsd_corr(s, cst, S);
    vmd_horn_matrix(S, N);
    vmd_jacobi4_t<false>(N, nullptr);                        // vmd_jacobi4's rotations; the eigenvectors are not needed
    double lam = N[0][0];
    for (int i = 1; i < 4; ++i) if (N[i][i] > lam) lam = N[i][i];
    double msd = ((Gp + Gq) - 2.0 * lam) / W;
    msd = msd < 0.0 ? 0.0 : msd;                            // a rigid copy rounds to -1e-13
    return (float)sqrt(msd);
}

// the shift that runs into chunk `chunk` of a (frame, context): the totals of the chunks in front of it
__device__ __forceinline__ void vmd_rmsd_carry_in(const int32_t* sh, int chunk, int run[3]) {
    run[0] = run[1] = run[2] = 0;
    for (int ch = 0; ch < chunk; ++ch) { run[0] += sh[4 * ch + 0]; run[1] += sh[4 * ch + 1]; run[2] += sh[4 * ch + 2]; }
}

// one block per (frame, context, chunk): the chunk's total link shift, the link to the previous chunk's last atom included
__global__ __launch_bounds__(VMD_SET_BLOCK) void k_rmsd_shift(vmd_rmsd_params_t p) {
    __shared__ int s_w[VMD_SET_WAVES][3];
    vmd_set_block_t w;
    if (!vmd_set_block(p.off, p.P, p.nchunk, w)) return;
    const vmd_set_frame_t sf = vmd_set_frame(p.f, w.b);
    const int32_t* set = p.set + w.s.k0;
    const float* mass = p.mass + w.s.k0;
    const int tid = threadIdx.x;
    int s[3] = {0, 0, 0};
#pragma unroll 1
    for (int g = 0; g < VMD_SET_STEPS; g += 4) {
        vmd_rmsd_atom_t q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = vmd_rmsd_load(sf.fr, set, mass, w.a0 + (g + u) * VMD_SET_BLOCK + tid, w.s.n);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            int nx, ny, nz;
            vmd_rmsd_link(q[u], sf, nx, ny, nz);
            s[0] += nx; s[1] += ny; s[2] += nz;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s[0] += vmd_shfl_xor_i32(s[0], o); s[1] += vmd_shfl_xor_i32(s[1], o); s[2] += vmd_shfl_xor_i32(s[2], o); }
    vmd_set_block_sum<int, 3>(s, s_w, p.shift + (size_t)blockIdx.x * 4);
}

// one block per (frame, context, chunk): carry-in from the earlier chunks' totals, the in-chunk prefix sum of the link shifts (a wave
// scan per step, the waves and steps joined through LDS), the sums per thread in registers, wave butterfly, the four waves through LDS.
// POSE: the same over trajectory frame 0 - stores u_a and sums W instead of C.
template <bool POSE>
__global__ __launch_bounds__(VMD_SET_BLOCK) void k_rmsd_moments(vmd_rmsd_params_t p) {
    __shared__ int s_tot[VMD_SET_STEPS][VMD_SET_WAVES][3];
    __shared__ double s_wave[VMD_SET_WAVES][VMD_RMSD_NSUM];
    vmd_set_block_t w;
    if (!vmd_set_block(p.off, p.P, p.nchunk, w)) return;
    const int n = w.s.n, a0 = w.a0;
    const vmd_set_frame_t sf = vmd_set_frame(p.f, w.b);
    const int32_t* set = p.set + w.s.k0;
    const float* mass = p.mass + w.s.k0;
    double* pose = p.pose + (size_t)w.s.k0 * 3;
    const int i0 = set[0];
    const double x0 = (double)sf.fr.x[i0], y0 = (double)sf.fr.y[i0], z0 = (double)sf.fr.z[i0];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the shift of every atom in front of the current step
    int run[3];
    vmd_rmsd_carry_in(p.shift + (size_t)w.bc * p.nchunk * 4, w.chunk, run);
    double s[VMD_RMSD_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    // VMD_RMSD_GROUP atoms per step: their loads first, the link shifts and their wave scans, one barrier, then the sums in atom order
#pragma unroll 1
    for (int g = 0; g < VMD_SET_STEPS; g += VMD_RMSD_GROUP) {
        vmd_rmsd_atom_t q[VMD_RMSD_GROUP];
        double u[VMD_RMSD_GROUP][3];
        int incl[VMD_RMSD_GROUP][3];
#pragma unroll
        for (int k = 0; k < VMD_RMSD_GROUP; ++k) {
            const int a = a0 + (g + k) * VMD_SET_BLOCK + tid;
            q[k] = vmd_rmsd_load(sf.fr, set, mass, a, n);
            const int aa = a < n ? a : 0;
            if (!POSE) { u[k][0] = pose[3 * aa + 0]; u[k][1] = pose[3 * aa + 1]; u[k][2] = pose[3 * aa + 2]; }
            else { u[k][0] = 0.0; u[k][1] = 0.0; u[k][2] = 0.0; }
        }
#pragma unroll
        for (int k = 0; k < VMD_RMSD_GROUP; ++k) {
            int tot[3];
            vmd_rmsd_wave_shift(q[k], sf, lane, incl[k], tot);
            if (lane == 0) { s_tot[g + k][wave][0] = tot[0]; s_tot[g + k][wave][1] = tot[1]; s_tot[g + k][wave][2] = tot[2]; }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < VMD_RMSD_GROUP; ++k) {
            int kk[3];
            vmd_rmsd_join(s_tot[g + k], wave, incl[k], run, kk);
            const int a = a0 + (g + k) * VMD_SET_BLOCK + tid;
            vmd_rmsd_add<POSE>(q[k].at, sf, x0, y0, z0, kk[0], kk[1], kk[2], u[k], (POSE && a < n) ? pose + 3 * (size_t)a : nullptr, s);
        }
    }
    vmd_set_wave_sum<VMD_RMSD_NSUM>(s);
    vmd_set_block_sum<double, VMD_RMSD_NSUM>(s, s_wave, p.partial + (size_t)blockIdx.x * VMD_RMSD_NSUM);
}

// one thread per (frame, context): the chunk sums in chunk order, then the value (POSE: the constants of the context)
template <bool POSE>
__global__ __launch_bounds__(64) void k_rmsd_finish(vmd_rmsd_params_t p) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= p.f.B * p.P) return;
    const int b = t / p.P, c = t - b * p.P;
    const int n = vmd_set_slice(p.off, c).n;
    double s[VMD_RMSD_NSUM];
    vmd_set_chunk_sum<VMD_RMSD_NSUM>(p.partial + (size_t)t * p.nchunk * VMD_RMSD_NSUM, n, s);
    double* cst = p.cst + (size_t)c * VMD_RMSD_NCONST;
    if (POSE) { cst[0] = s[13]; cst[1] = s[0]; cst[2] = s[1]; cst[3] = s[2]; cst[4] = s[3]; }
    else p.out[t] = b == p.zero_row ? 0.0f : vmd_rmsd_value(s, cst, n);
}

// populations of small sets (`rmsd(all) in residue(:)`): one wave per (frame, context), lane j holds atom j; the same sums in the same
// order as the block form gives for such a set (one chunk, one atom per thread, three empty waves), without shifts in memory.  The sums go
// to the partials (one "chunk" per set) and k_rmsd_finish forms the values, 64 sets per wave: a Jacobi iteration in lane 0 of every
// wave kept the other 63 lanes waiting (1.97 ms per 200 000 sets against 0.3 ms this way)
template <bool POSE>
__global__ __launch_bounds__(VMD_SET_BLOCK) void k_rmsd_small(vmd_rmsd_params_t p) {
    const int t = blockIdx.x * VMD_SET_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= p.f.B * p.P) return;   // the whole wave
    const int b = t / p.P, c = t - b * p.P;
    const vmd_set_slice_t sl = vmd_set_slice(p.off, c);
    const int n = sl.n;
    const vmd_set_frame_t sf = vmd_set_frame(p.f, b);
    const int32_t* set = p.set + sl.k0;
    double* pose = p.pose + (size_t)sl.k0 * 3;
    const int i0 = set[0];
    const double x0 = (double)sf.fr.x[i0], y0 = (double)sf.fr.y[i0], z0 = (double)sf.fr.z[i0];
    const vmd_rmsd_atom_t q = vmd_rmsd_load(sf.fr, set, p.mass + sl.k0, lane, n);
    const int aa = lane < n ? lane : 0;
    double u[3] = {0.0, 0.0, 0.0};
    if (!POSE) { u[0] = pose[3 * aa + 0]; u[1] = pose[3 * aa + 1]; u[2] = pose[3 * aa + 2]; }
    int nx, ny, nz, kx, ky, kz, tx, ty, tz;
    vmd_rmsd_link(q, sf, nx, ny, nz);
    vmd_wave_scan_i32(nx, lane, kx, tx);
    vmd_wave_scan_i32(ny, lane, ky, ty);
    vmd_wave_scan_i32(nz, lane, kz, tz);
    double s[VMD_RMSD_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    vmd_rmsd_add<POSE>(q.at, sf, x0, y0, z0, kx, ky, kz, u, (POSE && lane < n) ? pose + 3 * (size_t)lane : nullptr, s);
    vmd_set_wave_sum<VMD_RMSD_NSUM>(s);
    if (lane != 0) return;
#pragma unroll
    for (int k = 0; k < VMD_RMSD_NSUM; ++k) p.partial[(size_t)t * VMD_RMSD_NSUM + k] = vmd_set_small_sum(s[k]);
}

// ------------------------------------------------------------------------------------------------ K5e: rmsf

// The per-atom residual of rmsd's fit, d_a = R (e_a - ebar) - (u_a - ubar), accumulated over frames in fixed point: per atom the i64 sums
// of q(d_x), q(d_y), q(d_z) and the u64 sum of q2(|d|^2), q(v) = q2(v) = llrint(v 2^24) (D-RMSF-FIXED) - integers, so the record does not
// depend on the order in which frames, blocks, batches and ranks arrive.  The sums are rmsd's (k_rmsd_shift + k_rmsd_moments, or
// k_rmsd_small); k_rmsf_rotation forms R and the centroids from them, k_rmsf_accumulate / k_rmsf_small make the second pass over the set.
#define VMD_RMSF_NROT 15           // per (frame, context): R row-major (9), ebar (3), ubar (3)
#define VMD_RMSF_FRAMES 64         // most frames of one frame group of k_rmsf_accumulate (its LDS row of running shifts)
#define VMD_RMSF_ONE 16777216.0    // 2^24: one Angstrom (one square Angstrom) in quanta
#define VMD_RMSF_D2_MAX 1048576.0  // 2^20 A^2: where q2 saturates

struct vmd_rmsf_params_t {
    vmd_rmsd_params_t r;    // the frames, the set, the pose and its constants, the sums and chunk shifts of the batch, zero_row
    double* rot;            // [B][P][VMD_RMSF_NROT]
    uint64_t* acc;          // [off[P] + 1][4]: the record; row off[P] word 0 counts the frames
    int b0, nb;             // the frames of the batch this launch accumulates: [b0, b0 + nb)
    int groups;             // frame groups: group g takes frames b0 + g per .. b0 + (g + 1) per, per = ceil(nb / groups)
};

// one thread per (frame, context): the chunk sums in chunk order, then the rotation vmd_horn_rotation forms of the S of rmsd's finish and
// the two centroids.  D-RMSF-DEGENERATE sets get zeros (the second pass leaves them out by the same test).
__global__ __launch_bounds__(64) void k_rmsf_rotation(vmd_rmsf_params_t q) {
    const vmd_rmsd_params_t& p = q.r;
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= p.f.B * p.P) return;
    const int c = t % p.P;
    const int n = vmd_set_slice(p.off, c).n;
    const double* cst = p.cst + (size_t)c * VMD_RMSD_NCONST;
    double* o = q.rot + (size_t)t * VMD_RMSF_NROT;
    const double W = cst[0];
    if (n <= 1 || W == 0.0) {
        for (int k = 0; k < VMD_RMSF_NROT; ++k) o[k] = 0.0;
        return;
    }
    double s[VMD_RMSD_NSUM], S[3][3], R[9];
    vmd_set_chunk_sum<VMD_RMSD_NSUM>(p.partial + (size_t)t * p.nchunk * VMD_RMSD_NSUM, n, s);
    vmd_rmsd_corr(s, cst, S);
    vmd_horn_rotation_inline(S, R);
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = R[k];
    for (int k = 0; k < 3; ++k) { o[9 + k] = s[k] / W; o[12 + k] = cst[1 + k] / W; }
}

// the four quantised terms of one atom in one frame added to its registers
__device__ __forceinline__ void vmd_rmsf_add(const double* rot, double ex, double ey, double ez, const double u[3], long long a[4]) {
    const double px = ex - rot[9], py = ey - rot[10], pz = ez - rot[11];
    const double dx = ((rot[0] * px + rot[1] * py) + rot[2] * pz) - (u[0] - rot[12]);
    const double dy = ((rot[3] * px + rot[4] * py) + rot[5] * pz) - (u[1] - rot[13]);
    const double dz = ((rot[6] * px + rot[7] * py) + rot[8] * pz) - (u[2] - rot[14]);
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    a[0] += llrint(dx * VMD_RMSF_ONE); a[1] += llrint(dy * VMD_RMSF_ONE); a[2] += llrint(dz * VMD_RMSF_ONE);
    a[3] += llrint((d2 < VMD_RMSF_D2_MAX ? d2 : VMD_RMSF_D2_MAX) * VMD_RMSF_ONE);
}
__device__ __forceinline__ void vmd_rmsf_commit(uint64_t* row, const long long a[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) if (a[j]) atomicAdd((unsigned long long*)row + j, (unsigned long long)a[j]);
}
// the frames of group g: [fb, fb + nf)
__device__ __forceinline__ void vmd_rmsf_group(const vmd_rmsf_params_t& q, int g, int& fb, int& nf) {
    const int per = (q.nb + q.groups - 1) / q.groups;
    fb = q.b0 + g * per;
    nf = q.b0 + q.nb - fb;
    nf = nf < per ? nf : per;
    nf = nf < 0 ? 0 : nf;
}

// One block per (context, chunk, frame group).  A thread owns VMD_RMSD_GROUP atoms at a time: for each step of the chunk it walks the
// group's frames - per frame k_rmsd_moments' step (loads, vmd_rmsd_wave_shift, the waves joined through LDS, one barrier) gives e_a -,
// keeps the step's 4 x i64 per atom in registers, and issues their atomics behind the last frame.  What has run in front of the step in
// each frame stands in an LDS row, double-buffered by step like the wave totals by iteration: one barrier per (step, frame) is enough -
// both are read only behind the iteration's barrier, and written again no earlier than behind the next one.
__global__ __launch_bounds__(VMD_SET_BLOCK) void k_rmsf_accumulate(vmd_rmsf_params_t q) {
    __shared__ int s_tot[2][VMD_RMSD_GROUP][VMD_SET_WAVES][3];
    __shared__ int s_run[2][VMD_RMSF_FRAMES][3];
    const vmd_rmsd_params_t& p = q.r;
    const int g = blockIdx.x % q.groups, cc = blockIdx.x / q.groups;
    const int chunk = cc % p.nchunk, c = cc / p.nchunk;
    const vmd_set_slice_t sl = vmd_set_slice(p.off, c);
    const int n = sl.n, a0 = chunk * VMD_SET_CHUNK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int fb, nf;
    vmd_rmsf_group(q, g, fb, nf);
    if (cc == 0 && tid == 0 && nf > 0) atomicAdd((unsigned long long*)q.acc + 4 * (size_t)p.off[p.P], (unsigned long long)nf);
    if (a0 >= n || nf == 0 || n <= 1 || p.cst[(size_t)c * VMD_RMSD_NCONST] == 0.0) return;     // the whole block (D-RMSF-DEGENERATE: d = 0)
    const int32_t* set = p.set + sl.k0;
    const float* mass = p.mass + sl.k0;
    const double* pose = p.pose + (size_t)sl.k0 * 3;
    const int i0 = set[0];
    if (tid < nf) {
        int run[3];
        vmd_rmsd_carry_in(p.shift + ((size_t)(fb + tid) * p.P + c) * p.nchunk * 4, chunk, run);
        s_run[0][tid][0] = run[0]; s_run[0][tid][1] = run[1]; s_run[0][tid][2] = run[2];
    }
    __syncthreads();
    int it = 0;
#pragma unroll 1
    for (int st = 0; st < VMD_SET_STEPS; st += VMD_RMSD_GROUP) {
        if (a0 + st * VMD_SET_BLOCK >= n) break;                 // (the whole block: no atom of this step or a later one)
        const int par = (st / VMD_RMSD_GROUP) & 1;
        long long acc[VMD_RMSD_GROUP][4];
        double u[VMD_RMSD_GROUP][3];
#pragma unroll
        for (int k = 0; k < VMD_RMSD_GROUP; ++k) {
            const int a = a0 + (st + k) * VMD_SET_BLOCK + tid, aa = a < n ? a : 0;
            acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0;
            u[k][0] = pose[3 * aa + 0]; u[k][1] = pose[3 * aa + 1]; u[k][2] = pose[3 * aa + 2];
        }
#pragma unroll 1
        for (int f = 0; f < nf; ++f) {
            const int b = fb + f;
            if (b == p.zero_row) continue;                        // trajectory frame 0: d = 0 by construction, nothing to add
            const vmd_set_frame_t sf = vmd_set_frame(p.f, b);
            const double x0 = (double)sf.fr.x[i0], y0 = (double)sf.fr.y[i0], z0 = (double)sf.fr.z[i0];
            const double* rot = q.rot + ((size_t)b * p.P + c) * VMD_RMSF_NROT;
            vmd_rmsd_atom_t at[VMD_RMSD_GROUP];
            int incl[VMD_RMSD_GROUP][3];
#pragma unroll
            for (int k = 0; k < VMD_RMSD_GROUP; ++k) at[k] = vmd_rmsd_load(sf.fr, set, mass, a0 + (st + k) * VMD_SET_BLOCK + tid, n);
#pragma unroll
            for (int k = 0; k < VMD_RMSD_GROUP; ++k) {
                int tot[3];
                vmd_rmsd_wave_shift(at[k], sf, lane, incl[k], tot);
                if (lane == 0) { s_tot[it & 1][k][wave][0] = tot[0]; s_tot[it & 1][k][wave][1] = tot[1]; s_tot[it & 1][k][wave][2] = tot[2]; }
            }
            __syncthreads();
            // (read behind the barrier: thread 0 wrote this row at the end of the frame's iteration of the step before)
            int run[3] = {s_run[par][f][0], s_run[par][f][1], s_run[par][f][2]};
#pragma unroll
            for (int k = 0; k < VMD_RMSD_GROUP; ++k) {
                int kk[3];
                double ex, ey, ez;
                vmd_rmsd_join(s_tot[it & 1][k], wave, incl[k], run, kk);
                vmd_rmsd_offset(at[k].at, sf, x0, y0, z0, kk[0], kk[1], kk[2], ex, ey, ez);
                if (a0 + (st + k) * VMD_SET_BLOCK + tid < n) vmd_rmsf_add(rot, ex, ey, ez, u[k], acc[k]);
            }
            if (tid == 0) { s_run[par ^ 1][f][0] = run[0]; s_run[par ^ 1][f][1] = run[1]; s_run[par ^ 1][f][2] = run[2]; }
            it += 1;
        }
#pragma unroll
        for (int k = 0; k < VMD_RMSD_GROUP; ++k) {
            const int a = a0 + (st + k) * VMD_SET_BLOCK + tid;
            if (a < n) vmd_rmsf_commit(q.acc + 4 * ((size_t)sl.k0 + a), acc[k]);
        }
    }
}

// populations of small sets: one wave per (context, frame group), lane j owns atom j over the group's frames - k_rmsd_small's walk per
// frame, the same e_a, the same registers and atomics as the block form
__global__ __launch_bounds__(VMD_SET_BLOCK) void k_rmsf_small(vmd_rmsf_params_t q) {
    const vmd_rmsd_params_t& p = q.r;
    const int t = blockIdx.x * VMD_SET_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int g = t % q.groups, c = t / q.groups;
    if (c >= p.P) return;            // the whole wave
    int fb, nf;
    vmd_rmsf_group(q, g, fb, nf);
    if (c == 0 && lane == 0 && nf > 0) atomicAdd((unsigned long long*)q.acc + 4 * (size_t)p.off[p.P], (unsigned long long)nf);
    const vmd_set_slice_t sl = vmd_set_slice(p.off, c);
    const int n = sl.n;
    if (n <= 1 || p.cst[(size_t)c * VMD_RMSD_NCONST] == 0.0) return;     // D-RMSF-DEGENERATE
    const int32_t* set = p.set + sl.k0;
    const double* pose = p.pose + (size_t)sl.k0 * 3;
    const int i0 = set[0], aa = lane < n ? lane : 0;
    const double u[3] = {pose[3 * aa + 0], pose[3 * aa + 1], pose[3 * aa + 2]};
    long long acc[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (int f = 0; f < nf; ++f) {
        const int b = fb + f;
        if (b == p.zero_row) continue;
        const vmd_set_frame_t sf = vmd_set_frame(p.f, b);
        const double x0 = (double)sf.fr.x[i0], y0 = (double)sf.fr.y[i0], z0 = (double)sf.fr.z[i0];
        const vmd_rmsd_atom_t at = vmd_rmsd_load(sf.fr, set, p.mass + sl.k0, lane, n);
        int kk[3], tot[3];
        double ex, ey, ez;
        vmd_rmsd_wave_shift(at, sf, lane, kk, tot);
        vmd_rmsd_offset(at.at, sf, x0, y0, z0, kk[0], kk[1], kk[2], ex, ey, ez);
        if (lane < n) vmd_rmsf_add(q.rot + ((size_t)b * p.P + c) * VMD_RMSF_NROT, ex, ey, ez, u, acc);
    }
    if (lane < n) vmd_rmsf_commit(q.acc + 4 * ((size_t)sl.k0 + lane), acc);
}

// ------------------------------------------------------------------------------------------------ K12: hydrogen bonds

// A bond is one (donor pair j, acceptor k) combination: D = don[j] with its explicit hydrogen H = hyd[j], A the acceptor behind list entry k.
// Rule 1 (distance) is within()'s: wrapped positions, the SPEC S3 / S3t image, vmd_d2, vmd_within_hit with r_min = 0; e = (D - A) - shift is
// the delta the test squares.  Rule 2 (identity, by atom index), rules 3 and 4 (the hydrogen's image, the angle) are vmd_hbond_rule below.
// Every operation is fp32 and separately rounded (no fmaf here: the file is built with -ffp-contract=off).
__device__ __forceinline__ float vmd_dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// u = -h points from H to D, v = -e - h from H to A: the D-H...A angle is at least angle_min (>= 90 degrees) iff its cosine is at most
// cos(angle_min) <= 0, i.e. dot <= 0 and dot^2 >= c2 uu vv with c2 = cos^2(angle_min).  No root, no division, no acos.
__device__ __forceinline__ bool vmd_hbond_angle(float c2, float hx, float hy, float hz, float ex, float ey, float ez) {
    const float ux = -hx, uy = -hy, uz = -hz;
    const float vx = -ex - hx, vy = -ey - hy, vz = -ez - hz;
    const float uu = vmd_dot3(ux, uy, uz, ux, uy, uz), vv = vmd_dot3(vx, vy, vz, vx, vy, vz), dot = vmd_dot3(ux, uy, uz, vx, vy, vz);
    return uu > 0.0f && vv > 0.0f && dot <= 0.0f && dot * dot >= c2 * (uu * vv);
}

// one donor pair as its lane holds it: the atoms, and h = the minimum image of (H - D) from the RAW frame (the image function of distance())
struct vmd_hbond_pair_t { int d, h; float hx, hy, hz; };
__device__ __forceinline__ vmd_hbond_pair_t vmd_hbond_pair(const vmd_box_t& bx, const float* fx, const float* fy, const float* fz, int d, int h) {
    vmd_hbond_pair_t q;
    q.d = d; q.h = h;
    q.hx = fx[h] - fx[d]; q.hy = fy[h] - fy[d]; q.hz = fz[h] - fz[d];
    vmd_mi3_rintf(bx, q.hx, q.hy, q.hz);
    return q;
}
// rules 2 - 4 for a distance hit of the pair against acceptor atom `a` at delta e
__device__ __forceinline__ bool vmd_hbond_rule(const vmd_hbond_pair_t& q, float c2, int a, float ex, float ey, float ez) {
    return a != q.d && a != q.h && vmd_hbond_angle(c2, q.hx, q.hy, q.hz, ex, ey, ez);
}

__device__ __forceinline__ void vmd_atomic_add_u64(uint64_t* p, uint64_t v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }
// (the SIMT emulator under tests/emu runs one lane at a time and its header has no atomicMin: there the claim is the plain compare and
// store its other atomics are)
__device__ __forceinline__ void vmd_atomic_min_u32(uint32_t* p, uint32_t v) {
#ifdef __HIPCC__
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}

// The lanes' values summed over the wave (xor shuffles), ONE atomic of the wave's leader where the sum is not zero.  Every lane of the wave
// calls them.
__device__ __forceinline__ void vmd_wave_add_u32(unsigned* dst, unsigned v) {
    int tot = (int)v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot += vmd_shfl_xor_i32(tot, o);
    if ((threadIdx.x & 63) == 0 && tot) atomicAdd(dst, (unsigned)tot);
}
__device__ __forceinline__ void vmd_wave_add_u64(uint64_t* dst, uint64_t v) {
    uint64_t tot = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)vmd_shfl_xor_i32((int)(uint32_t)tot, o), hi = (uint32_t)vmd_shfl_xor_i32((int)(uint32_t)(tot >> 32), o);
        tot += ((uint64_t)hi << 32) | lo;
    }
    if ((threadIdx.x & 63) == 0 && tot) vmd_atomic_add_u64(dst, tot);
}

// what a lane has found goes out the same way from the walk and from all pairs: the lanes' bond counts summed over the wave into ONE u32
// atomic on the frame's count, one u64 atomic per lane with bonds into its donor row.  (The acceptor rows take one atomic per bond, where
// the bond is found.)  Every lane of the wave calls it.
__device__ __forceinline__ void vmd_hbond_commit(unsigned* frame_count, uint64_t* donor_row, unsigned n) {
    if (n) vmd_atomic_add_u64(donor_row, n);
    vmd_wave_add_u32(frame_count, n);
}

// An entry's own slots in a cell-sorted copy (cs: its cell_start, xr / yr / zr: its rows, n entries): visit(slot), in ascending order, for
// every slot in the run of the entry's cell whose three coordinates equal the entry's wrapped ones bit for bit - vmd_cell_of gives the
// values the build binned and stored -, until it returns true.  (A table is never trusted beyond the copy it indexes.)
template <class Visit>
__device__ __forceinline__ void vmd_own_slots(const uint32_t* cs, const float* xr, const float* yr, const float* zr, uint32_t n,
                                              uint32_t cell, float x, float y, float z, Visit visit) {
    const int bx_ = __float_as_int(x), by_ = __float_as_int(y), bz_ = __float_as_int(z);
    uint32_t s0 = cs[cell], s1 = cs[cell + 1];
    if (s1 > n) s1 = n;
    for (uint32_t s = s0; s < s1; ++s)
        if (__float_as_int(xr[s]) == bx_ && __float_as_int(yr[s]) == by_ && __float_as_int(zr[s]) == bz_ && visit(s)) break;
}

// The identity of a cell-sorted copy, recovered without touching the cell build: one lane per list entry t.  The lane claims every slot of
// its own (vmd_own_slots) with atomicMin (vmd_atomic_min_u32).  ident is
// u32[B][nsel_pad], preset to 0xffffffff by the launcher.  DECISION(D-HB-COINCIDENT): entries that coincide bit for bit in a frame share
// their slots, and every one of those slots answers as the LOWEST such entry; a slot left at 0xffffffff after the pass is a bug.
struct vmd_sorted_atoms_params_t {
    vmd_cells_params_t c;       // the selection as its cell build read it: raw frame, the GRID's boxes, pbc, index list, grid (no outputs)
    const uint32_t* cell_start; const float* sorted;
    uint32_t* ident; const uint32_t* skip;
};
__global__ __launch_bounds__(256) void k_sorted_atoms(vmd_sorted_atoms_params_t p) {
    if (p.skip && *p.skip) return;       // a cell build of this batch overflowed a bucket: the table it would read is void
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.c.nsel) return;
    float xw, yw, zw;
    const uint32_t cell = vmd_cell_of(p.c, b, t, xw, yw, zw);
    const uint32_t* cs = p.cell_start + (size_t)b * (p.c.grid.ncell + 1);
    const float* xr = p.sorted + (size_t)b * 3 * p.c.nsel_pad;
    const float* yr = xr + p.c.nsel_pad;
    const float* zr = yr + p.c.nsel_pad;
    uint32_t* id = p.ident + (size_t)b * p.c.nsel_pad;
    vmd_own_slots(cs, xr, yr, zr, (uint32_t)p.c.nsel, cell, xw, yw, zw, [&](uint32_t s) { vmd_atomic_min_u32(&id[s], (uint32_t)t); return false; });
}

struct vmd_hbond_atoms_params_t {
    vmd_cells_params_t c;       // the donors as a cell build would read them: raw frame, the GRID's boxes, pbc, the donor list, grid (no outputs)
    vmd_within_walk_params_t k; // the cell-sorted copy of the acceptors
    const float* fboxes;        // the frames' own cells: the hydrogen's image is taken in them (the grid's differ on open axes)
    const int32_t* hyd; const int32_t* accl; int nacc;
    const uint32_t* ident;      // k_sorted_atoms' table of the acceptor copy, u32[B][k.nref_pad]
    float c2;
    unsigned* count; uint64_t* acc;      // u32[B]; u64[nsel + nacc + 1]: donor rows, acceptor rows (the frames row is k_hbond_finish's)
    const uint32_t* skip;
};

// The walk, one lane per donor pair j in list order, D standing where vmd_walk_lane puts it.  Every distance hit is put to rules
// 2 - 4 (rule 4 first, see below).  Lanes of a wave are spatially unrelated, as in k_within_atoms: hits are few (about ten per donor at 3.5 A in
// water) and are taken where they are found, without compaction.
__global__ __launch_bounds__(256) void k_hbond_atoms(vmd_hbond_atoms_params_t p) {
    if (p.skip && *p.skip) return;       // a cell build of this batch overflowed a bucket: the host repeats the batch, nothing may be added
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const vmd_within_walk_t k = vmd_within_walk_setup(p.c.boxes, b, p.c.pbc, p.c.grid, p.k);
    unsigned n = 0;
    if (t < p.c.nsel) {
        const vmd_walk_lane_t l = vmd_walk_lane(p.c, k, b, t);
        const float* fx = p.c.xyz + (size_t)b * p.c.frame_stride;
        const vmd_hbond_pair_t q = vmd_hbond_pair(vmd_load_box(p.fboxes, b, p.c.pbc), fx, fx + p.c.row_stride, fx + 2 * p.c.row_stride,
                                                  p.c.sel[t], p.hyd[t]);
        const uint32_t* id = p.ident + (size_t)b * p.k.nref_pad;
        uint64_t* acc_rows = p.acc + p.c.nsel;
        const int nacc = p.nacc;
        const int32_t* accl = p.accl;
        const float c2 = p.c2;
        vmd_within_walk_each(k, l.py, l.pz, l.x, l.y, l.z, [&](unsigned j, float ex, float ey, float ez) {
            // the angle first: it needs no memory and drops all but a few per cent of the distance hits (the donor itself at d = 0 among
            // them), so the two dependent loads of the identity are paid by what is nearly a bond.  The conjunction is the same.
            if (!vmd_hbond_angle(c2, q.hx, q.hy, q.hz, ex, ey, ez)) return false;
            const uint32_t a = id[j];
            if (a >= (uint32_t)nacc) return false;    // (an unclaimed slot would be a bug of k_sorted_atoms; it is never an index)
            const int aa = accl[a];
            if (aa != q.d && aa != q.h) { vmd_atomic_add_u64(acc_rows + a, 1); n += 1; }
            return false;
        });
    }
    vmd_hbond_commit(p.count + b, p.acc + (t < p.c.nsel ? t : 0), n);
}

// The coincidence table of every all-pairs route, which has no sorted copy to ask (D-HB-COINCIDENT, D-SASA-COINCIDENT, D-CT-COINCIDENT):
// canon[b][k] = the lowest entry of the list whose wrapped coordinates in frame b equal entry k's bit for bit (k itself where nothing
// coincides) - what k_sorted_atoms' table answers for k's slot.  One lane per entry over vmd_all_pairs, up to the block's highest entry;
// the lane compares the staged bit patterns and leaves at its first match or at itself.
struct vmd_canon_params_t {
    const float* xyz; size_t frame_stride; size_t row_stride;
    const float* boxes; uint32_t pbc;
    const int32_t* list; int n;
    uint32_t* canon;            // u32[B][n]
    const uint32_t* skip;
};
__global__ __launch_bounds__(256) void k_canon_entries(vmd_canon_params_t p) {
    __shared__ float s_r[3][256];
    if (p.skip && *p.skip) return;
    const int b = blockIdx.y;
    const int k = blockIdx.x * 256 + threadIdx.x;
    const float* fx = p.xyz + (size_t)b * p.frame_stride;
    const float* fy = fx + p.row_stride;
    const float* fz = fy + p.row_stride;
    const vmd_box_t bx = vmd_load_box(p.boxes, b, p.pbc);
    const bool valid = k < p.n;
    float xi = 0.0f, yi = 0.0f, zi = 0.0f;
    if (valid) { const int a = p.list[k]; vmd_pair_coords(bx, fx[a], fy[a], fz[a], xi, yi, zi); }
    const int bxi = __float_as_int(xi), byi = __float_as_int(yi), bzi = __float_as_int(zi);
    int found = k;
    const int last = blockIdx.x * 256 + 255 < p.n ? blockIdx.x * 256 + 255 : p.n - 1;       // the block's highest entry
    vmd_all_pairs<256>(s_r, bx, fx, fy, fz, p.list, last + 1, 0, valid, xi, yi, zi, [](int, int) {},
        [&](int jj, int pos, float, float, float) {
            if (pos >= k) return true;
            if (__float_as_int(s_r[0][jj]) != bxi || __float_as_int(s_r[1][jj]) != byi || __float_as_int(s_r[2][jj]) != bzi) return false;
            found = pos;
            return true;
        });
    if (valid) p.canon[(size_t)b * p.n + k] = (uint32_t)found;
}

struct vmd_hbond_brute_params_t {
    const float* xyz; size_t frame_stride; size_t row_stride;
    const float* boxes; uint32_t pbc;
    const int32_t* don; const int32_t* hyd; int npairs; const int32_t* accl; int nacc;
    const uint32_t* canon;      // k_canon_entries' table of the acceptors, u32[B][nacc]
    vmd_within_test_t w; float c2;
    unsigned* count; uint64_t* acc; const uint32_t* skip;
    uint32_t* list; uint32_t list_cap; unsigned* list_count;      // LIST: u32[list_cap][2] = {pair j, acceptor list position}, the bonds found
};

// All pairs from the raw frame: one lane per donor pair over vmd_all_pairs, the acceptors staged with their canonical entry and its atom,
// identity = the list position (through canon).  The same rules, the same outputs as the walk.  LIST: the bonds go to a capped buffer
// through a counter instead (vmd_eval_hbond_pairs), nothing is accumulated.
template <bool LIST>
__global__ __launch_bounds__(256) void k_hbond_brute(vmd_hbond_brute_params_t p) {
    __shared__ float s_r[3][256];
    __shared__ uint32_t s_k[256];
    __shared__ int s_a[256];
    if (p.skip && *p.skip) return;
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const float* fx = p.xyz + (size_t)b * p.frame_stride;
    const float* fy = fx + p.row_stride;
    const float* fz = fy + p.row_stride;
    const vmd_box_t bx = vmd_load_box(p.boxes, b, p.pbc);
    const bool valid = t < p.npairs;
    float xi = VMD_FAR, yi = VMD_FAR, zi = VMD_FAR;
    vmd_hbond_pair_t q{0, 0, 0.0f, 0.0f, 0.0f};
    if (valid) {
        q = vmd_hbond_pair(bx, fx, fy, fz, p.don[t], p.hyd[t]);
        vmd_pair_coords(bx, fx[q.d], fy[q.d], fz[q.d], xi, yi, zi);
    }
    const uint32_t* canon = p.canon + (size_t)b * p.nacc;
    unsigned n = 0;
    vmd_all_pairs<256>(s_r, bx, fx, fy, fz, p.accl, p.nacc, 0, valid, xi, yi, zi,
        [&](int jj, int pos) { s_k[jj] = canon[pos]; s_a[jj] = p.accl[s_k[jj]]; },
        [&](int jj, int pos, float ex, float ey, float ez) {
            if (!vmd_within_hit(p.w, vmd_d2(ex, ey, ez)) || !vmd_hbond_rule(q, p.c2, s_a[jj], ex, ey, ez)) return false;
            if (LIST) {
                const unsigned slot = atomicAdd(p.list_count, 1u);
                if (slot < p.list_cap) { p.list[2 * (size_t)slot] = (uint32_t)t; p.list[2 * (size_t)slot + 1] = (uint32_t)pos; }
            } else {
                vmd_atomic_add_u64(p.acc + p.npairs + s_k[jj], 1);
                n += 1;
            }
            return false;
        });
    if (!LIST) vmd_hbond_commit(p.count + b, p.acc + (valid ? t : 0), n);
}

// the launcher's finishing step, behind the last launch over a frame group: the counts as the temporal rows, the frames row bumped once per
// frame - under the overflow flag like everything above
__global__ __launch_bounds__(256) void k_hbond_finish(const unsigned* count, int B, float* out, uint64_t* frames_row, const uint32_t* skip) {
    if (skip && *skip) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B) out[i] = (float)count[i];
    if (i == 0) *frames_row += (uint64_t)B;
}

// ------------------------------------------------------------------------------------------------ K13: solvent-accessible surface area

// Shrake-Rupley.  Measured entry i (atom meas[i], R_i = radius + probe) carries P points R_i u_k on its sphere; n_i counts the points
// that lie inside no neighbour's sphere.  Environment entry j (through its canonical entry: D-SASA-COINCIDENT) is a neighbour iff
//   1. the pair passes within(r_cut, .)'s distance test, r_cut = 2 max(R) - wrapped positions, the S3 / S3t image, vmd_d2, vmd_within_hit
//      with r_min = 0; e = (i - j) - shift is the delta that test squares, d2 the value it compared;
//   2. d2 < s s strictly, s = R_i + R_j;
//   3. j's atom is not i's atom, by index.
// Point k is buried by neighbour j iff (u_kx e_x + u_ky e_y) + u_kz e_z < t_ij, t_ij = ((R_j R_j - R_i R_i) - d2) / (R_i + R_i): this is
// |R_i u_k + e|^2 < R_j^2 rearranged.  fp32, every operation rounded on its own.  The area is integer: w_i = llround(4 pi R_i^2 / P * 2^20)
// formed on the host, the frame's total the u64 sum of n_i w_i - atomics in any order give the same bits.
// the point table u32-aligned in LDS, one row of four floats per point: k is uniform over the wave, a read is one broadcast
__device__ __forceinline__ void vmd_sasa_stage_points(float (&s_u)[VMD_SASA_POINTS_MAX][4], const float* points, int P) {
    for (int k = threadIdx.x; k < P; k += blockDim.x) {
        s_u[k][0] = points[3 * k]; s_u[k][1] = points[3 * k + 1]; s_u[k][2] = points[3 * k + 2]; s_u[k][3] = 0.0f;
    }
    __syncthreads();
}

// a lane's P point bits, W words of 32: bit set = not buried so far
template <int W>
__device__ __forceinline__ void vmd_sasa_mask_full(uint32_t (&m)[W], int P) {
#pragma unroll
    for (int w = 0; w < W; ++w) { const int n = P - 32 * w; m[w] = n >= 32 ? 0xffffffffu : n > 0 ? (1u << n) - 1u : 0u; }
}
template <int W>
__device__ __forceinline__ uint32_t vmd_sasa_mask_any(const uint32_t (&m)[W]) {
    uint32_t v = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) v |= m[w];
    return v;
}
template <int W>
__device__ __forceinline__ unsigned vmd_sasa_mask_count(const uint32_t (&m)[W]) {
    unsigned n = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) n += (unsigned)__popcll((unsigned long long)m[w]);
    return n;
}
// D-SASA-POINT for one neighbour: the word index is a compile-time constant (the words stay in registers), a word without points left is
// passed over
template <int W>
__device__ __forceinline__ void vmd_sasa_bury(uint32_t (&m)[W], int P, const float (&s_u)[VMD_SASA_POINTS_MAX][4], float ex, float ey,
                                              float ez, float t) {
#pragma unroll
    for (int w = 0; w < W; ++w) {
        uint32_t mw = m[w];
        if (!mw) continue;
        const int n = P - 32 * w < 32 ? P - 32 * w : 32;
        for (int kk = 0; kk < n; ++kk) {
            const float* u = s_u[32 * w + kk];
            if ((u[0] * ex + u[1] * ey) + u[2] * ez < t) mw &= ~(1u << kk);
        }
        m[w] = mw;
    }
}
// rules 2 and 3 and the point tests for one distance hit, the same from the walk and from all pairs.  smax2 = fl(fl(R_i + max R)^2) bounds
// fl(s s) from above (rounding is monotonic), so the test against it drops a hit before anything is loaded.
struct vmd_sasa_entry_t { int atom; float R, R2, twoR, smax2; };
__device__ __forceinline__ vmd_sasa_entry_t vmd_sasa_entry(int atom, float R, float rmax_env) {
    vmd_sasa_entry_t q;
    q.atom = atom; q.R = R; q.R2 = R * R; q.twoR = R + R;
    const float sm = R + rmax_env;
    q.smax2 = sm * sm;
    return q;
}
template <int W>
__device__ __forceinline__ void vmd_sasa_neighbour(uint32_t (&m)[W], int P, const float (&s_u)[VMD_SASA_POINTS_MAX][4],
                                                   const vmd_sasa_entry_t& q, int atom_j, float Rj, float d2, float ex, float ey, float ez) {
    const float s = q.R + Rj;
    if (!(d2 < s * s) || atom_j == q.atom) return;
    const float t = ((Rj * Rj - q.R2) - d2) / q.twoR;
    vmd_sasa_bury(m, P, s_u, ex, ey, ez, t);
}

// what a lane has found goes out the same way from the walk and from all pairs: one u64 atomic per lane with points into its row, the lanes'
// n_i w_i summed over the wave into ONE u64 atomic on the frame's total.  Every lane of the wave calls it.
__device__ __forceinline__ void vmd_sasa_commit(uint64_t* frame_total, uint64_t* row, unsigned n, uint32_t weight) {
    if (n) vmd_atomic_add_u64(row, n);
    vmd_wave_add_u64(frame_total, (uint64_t)n * (uint64_t)weight);
}

struct vmd_sasa_atoms_params_t {
    vmd_cells_params_t c;       // the measured entries as a cell build would read them: raw frame, the GRID's boxes, pbc, their list, grid (no outputs)
    vmd_within_walk_params_t k; // the cell-sorted copy of the environment, the test of within(r_cut, .)
    const int32_t* envl; int nenv;
    const uint32_t* ident;      // k_sorted_atoms' table of the environment copy, u32[B][k.nref_pad]
    const float* r_meas; const float* r_env; float rmax_env;      // R = radius + probe per list entry; the largest of the environment
    const uint32_t* weight;     // w_i per measured entry
    const float* points; int npoints;      // f32[npoints][3]
    uint64_t* total; uint64_t* acc;        // u64[B] (zeroed by the call); u64[nsel + 1]: the rows (the frames row is k_sasa_finish's)
    const uint32_t* skip;
};

// The walk, one lane per measured entry in list order, standing where vmd_walk_lane puts it.  The lane keeps its point bits in W
// registers.  Lanes of a wave are spatially unrelated: a neighbour is taken where it is found, without compaction.
template <int W>
__global__ __launch_bounds__(256) void k_sasa_atoms(vmd_sasa_atoms_params_t p) {
    __shared__ float s_u[VMD_SASA_POINTS_MAX][4];
    if (p.skip && *p.skip) return;       // a cell build of this batch overflowed a bucket: the host repeats the batch, nothing may be added
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int P = p.npoints;
    vmd_sasa_stage_points(s_u, p.points, P);
    const vmd_within_walk_t k = vmd_within_walk_setup(p.c.boxes, b, p.c.pbc, p.c.grid, p.k);
    unsigned n = 0;
    uint32_t weight = 0;
    if (t < p.c.nsel) {
        const vmd_walk_lane_t l = vmd_walk_lane(p.c, k, b, t);
        const vmd_sasa_entry_t q = vmd_sasa_entry(p.c.sel[t], p.r_meas[t], p.rmax_env);
        const uint32_t* id = p.ident + (size_t)b * p.k.nref_pad;
        const int nenv = p.nenv;
        const int32_t* envl = p.envl;
        const float* r_env = p.r_env;
        uint32_t m[W];
        vmd_sasa_mask_full(m, P);
        vmd_within_walk_each(k, l.py, l.pz, l.x, l.y, l.z, [&](unsigned j, float ex, float ey, float ez) {
            // rule 2 against the largest environment radius first: it needs no memory.  A lane whose points are all buried has nothing
            // left to clear (and walks on all the same)
            const float d2 = vmd_d2(ex, ey, ez);
            if (!(d2 < q.smax2) || !vmd_sasa_mask_any(m)) return false;
            const uint32_t a = id[j];
            if (a >= (uint32_t)nenv) return false;    // (an unclaimed slot would be a bug of k_sorted_atoms; it is never an index)
            vmd_sasa_neighbour(m, P, s_u, q, envl[a], r_env[a], d2, ex, ey, ez);
            return false;
        });
        n = vmd_sasa_mask_count(m);
        weight = p.weight[t];
    }
    vmd_sasa_commit(p.total + b, p.acc + (t < p.c.nsel ? t : 0), n, weight);
}

struct vmd_sasa_brute_params_t {
    const float* xyz; size_t frame_stride; size_t row_stride;
    const float* boxes; uint32_t pbc;
    const int32_t* meas; int nmeas; const int32_t* envl; int nenv;
    const uint32_t* canon;      // k_canon_entries' table of the environment, u32[B][nenv]
    const float* r_meas; const float* r_env; float rmax_env;
    const uint32_t* weight;
    const float* points; int npoints;
    vmd_within_test_t w;        // within(r_cut, .)
    uint64_t* total; uint64_t* acc; const uint32_t* skip;
    uint32_t* counts;           // LIST: u32[nmeas], n_i of the one frame
};

// All pairs from the raw frame: one lane per measured entry over vmd_all_pairs, the environment staged with its canonical entry's
// atom and R.  The same rules, the same outputs as the walk.  LIST: the point counts of the frame go to counts[nmeas] instead
// (vmd_eval_sasa_atoms), nothing is accumulated.
template <bool LIST>
__global__ __launch_bounds__(256) void k_sasa_brute(vmd_sasa_brute_params_t p) {
    __shared__ float s_u[VMD_SASA_POINTS_MAX][4];
    __shared__ float s_r[3][256];
    __shared__ float s_R[256];
    __shared__ int s_a[256];
    if (p.skip && *p.skip) return;
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int P = p.npoints;
    vmd_sasa_stage_points(s_u, p.points, P);
    const float* fx = p.xyz + (size_t)b * p.frame_stride;
    const float* fy = fx + p.row_stride;
    const float* fz = fy + p.row_stride;
    const vmd_box_t bx = vmd_load_box(p.boxes, b, p.pbc);
    const bool valid = t < p.nmeas;
    float xi = VMD_FAR, yi = VMD_FAR, zi = VMD_FAR;
    vmd_sasa_entry_t q = vmd_sasa_entry(-1, 1.0f, 1.0f);
    constexpr int W = VMD_SASA_POINTS_MAX / 32;
    uint32_t m[W];
    vmd_sasa_mask_full(m, valid ? P : 0);
    if (valid) {
        q = vmd_sasa_entry(p.meas[t], p.r_meas[t], p.rmax_env);
        vmd_pair_coords(bx, fx[q.atom], fy[q.atom], fz[q.atom], xi, yi, zi);
    }
    const uint32_t* canon = p.canon + (size_t)b * p.nenv;
    vmd_all_pairs<256>(s_r, bx, fx, fy, fz, p.envl, p.nenv, 0, valid, xi, yi, zi,
        [&](int jj, int pos) { const uint32_t kk = canon[pos]; s_a[jj] = p.envl[kk]; s_R[jj] = p.r_env[kk]; },
        [&](int jj, int, float ex, float ey, float ez) {
            const float d2 = vmd_d2(ex, ey, ez);
            if (vmd_within_hit(p.w, d2) && d2 < q.smax2 && vmd_sasa_mask_any(m))
                vmd_sasa_neighbour(m, P, s_u, q, s_a[jj], s_R[jj], d2, ex, ey, ez);
            return false;
        });
    const unsigned n = vmd_sasa_mask_count(m);
    if (LIST) { if (valid) p.counts[t] = n; }
    else vmd_sasa_commit(p.total + b, p.acc + (valid ? t : 0), n, valid ? p.weight[t] : 0u);
}

// the launcher's finishing step, behind the last launch over a frame group: the totals as the temporal rows, (float)(total 2^-20), the frames
// row bumped once per frame - under the overflow flag like everything above
__global__ __launch_bounds__(256) void k_sasa_finish(const uint64_t* total, int B, float* out, uint64_t* frames_row, const uint32_t* skip) {
    if (skip && *skip) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < B) out[i] = (float)((double)total[i] * 9.5367431640625e-07);
    if (i == 0) *frames_row += (uint64_t)B;
}

// ------------------------------------------------------------------------------------------------ K14: residue contact maps

// One list of entries (atom, group) against itself.  Groups g < h with h - g >= min_sep are in contact in a frame when an entry acting for g
// and an entry acting for h pass within()'s pair distance (rule 1 of K12, word for word).  DECISION(D-CT-COINCIDENT): an entry acts - in the
// lane and as a hit alike - for the group of the LOWEST list entry whose wrapped coordinates coincide with its own bit for bit, so a pair is
// the same pair from either side.  Every hit of the walk ends in ONE bit of the frame's row of a bit matrix, u32[B][W]: bit p & 31 of word
// p >> 5 is the pair with the condensed index p (SciPy's pdist order).  Bits are idempotent: however many atom pairs stand behind a group
// pair, and from whichever side they are found, the row holds the same word.
__device__ __forceinline__ uint32_t vmd_contact_pair(uint32_t G, uint32_t g, uint32_t h) { return g * (2u * G - g - 1u) / 2u + (h - g - 1u); }
// (the SIMT emulator's header has __popcll alone)
__device__ __forceinline__ unsigned vmd_popc_u32(uint32_t v) { return (unsigned)__popcll((unsigned long long)v); }

// the plain load first: a residue pair in contact has several atom pairs in range, met by both of their lanes, so most hits find their bit
// set and end here.  A stale zero (another XCD's line in this CU's L1) costs one redundant atomic, never a wrong bit.
__device__ __forceinline__ void vmd_contact_set(uint32_t* row, uint32_t p) {
    uint32_t* w = row + (p >> 5);
    const uint32_t m = 1u << (p & 31u);
    if (!(*w & m)) atomicOr(w, m);
}
// groups a, b of an entry pair in range -> the bit, where they are a pair at all
__device__ __forceinline__ void vmd_contact_hit(uint32_t* row, uint32_t G, uint32_t min_sep, uint32_t a, uint32_t b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    if (hi - lo >= min_sep) vmd_contact_set(row, vmd_contact_pair(G, lo, hi));
}

struct vmd_contact_atoms_params_t {
    vmd_cells_params_t c;       // the entries as their cell build read them: raw frame, the GRID's boxes, pbc, the list, grid (no outputs)
    vmd_within_walk_params_t k; // the cell-sorted copy of the SAME list, the test of within(r_cut, .)
    const int32_t* grp; uint32_t ngroups, min_sep;
    const uint32_t* ident;      // k_sorted_atoms' table of the copy, u32[B][k.nref_pad]
    uint32_t* bits; uint32_t W; // u32[B][W], cleared by the launcher
    const uint32_t* skip;
};

// The walk, one lane per entry in list order, standing where vmd_walk_lane puts it.  The lane first finds ITSELF in its cell's run of the
// sorted copy (the first of vmd_own_slots): that slot's identity is the entry the lane acts for.  A hit is kept from the lower group's side only; the other lane finds the same pair from its side.
// LDS (the measured variant): the block first ORs its hits into LDS - the bit rows of the groups its 256 entries act for are ONE run of
// pair indices, p0(gmin) .. p0(gmax + 1) - 1 with p0(g) = g (2G - g - 1) / 2, because a hit is kept from the lower group's side - and
// then flushes the nonzero words with one atomicOr each.  A block whose run does not fit VMD_CONTACT_LDS_WORDS (scattered groups, many
// groups) takes the direct path, block-uniformly.
#define VMD_CONTACT_LDS_WORDS 4096
template <bool LDS>
__global__ __launch_bounds__(256) void k_contact_atoms(vmd_contact_atoms_params_t p) {
    __shared__ uint32_t s_bits[LDS ? VMD_CONTACT_LDS_WORDS : 1];
    __shared__ uint32_t s_rng[2];
    if (p.skip && *p.skip) return;       // a cell build of this batch overflowed a bucket: the table and the copy are void
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const bool valid = t < p.c.nsel;
    if (!LDS && !valid) return;
    const vmd_within_walk_t k = vmd_within_walk_setup(p.c.boxes, b, p.c.pbc, p.c.grid, p.k);
    const uint32_t* id = p.ident + (size_t)b * p.k.nref_pad;
    const uint32_t n = (uint32_t)p.c.nsel;
    const int32_t* grp = p.grp;
    const uint32_t G = p.ngroups, min_sep = p.min_sep;
    float xi = 0.0f, yi = 0.0f, zi = 0.0f;
    int py = 0, pz = 0;
    uint32_t gl = 0;
    if (valid) {
        const vmd_walk_lane_t l = vmd_walk_lane(p.c, k, b, t);
        xi = l.x; yi = l.y; zi = l.z; py = l.py; pz = l.pz;
        uint32_t me = (uint32_t)t;
        vmd_own_slots(k.csr, k.xr, k.yr, k.zr, n, l.cell, xi, yi, zi, [&](uint32_t s) { if (id[s] < n) me = id[s]; return true; });
        gl = (uint32_t)grp[me];
    }
    uint32_t* row = p.bits + (size_t)b * p.W;
    uint32_t w0 = 0, nw = 0;             // LDS: the block's run of words of the row, nw = 0 where it takes the direct path
    if (LDS) {
        if (threadIdx.x == 0) { s_rng[0] = 0xffffffffu; s_rng[1] = 0u; }
        __syncthreads();
        if (valid) { vmd_atomic_min_u32(&s_rng[0], gl); atomicMax(&s_rng[1], gl); }
        __syncthreads();
        const uint32_t gmin = s_rng[0], gmax = s_rng[1];
        const uint32_t pa = gmin * (2u * G - gmin - 1u) / 2u, pb = (gmax + 1u) * (2u * G - gmax - 2u) / 2u;
        if (pb > pa) {
            w0 = pa >> 5;
            nw = ((pb - 1u) >> 5) - w0 + 1u;
            if (nw > VMD_CONTACT_LDS_WORDS) nw = 0;
        }
        for (uint32_t i = threadIdx.x; i < nw; i += 256) s_bits[i] = 0u;
        __syncthreads();
    }
    if (valid)
        vmd_within_walk_each(k, py, pz, xi, yi, zi, [&](unsigned j, float, float, float) {
            const uint32_t a = id[j];
            if (a >= n) return false;    // (an unclaimed slot would be a bug of k_sorted_atoms; it is never an index)
            const uint32_t go = (uint32_t)grp[a];
            if (!(go > gl && go - gl >= min_sep)) return false;
            const uint32_t pp = vmd_contact_pair(G, gl, go);
            if (LDS && nw) vmd_contact_set(s_bits, pp - (w0 << 5));
            else vmd_contact_set(row, pp);
            return false;
        });
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nw; i += 256) {
            const uint32_t v = s_bits[i];
            if (v && (row[w0 + i] & v) != v) atomicOr(row + w0 + i, v);
        }
    }
}

struct vmd_contact_brute_params_t {
    const float* xyz; size_t frame_stride; size_t row_stride;
    const float* boxes; uint32_t pbc;
    const int32_t* ent; const int32_t* grp; int nent; uint32_t ngroups, min_sep;
    const uint32_t* canon;      // k_canon_entries' table of the list, u32[B][nent]
    vmd_within_test_t w;        // within(r_cut, .)
    uint32_t* bits; uint32_t W; const uint32_t* skip;
};

// All pairs from the raw frame: one lane per entry over vmd_all_pairs, the list staged with the group of every entry's canonical entry.
// The upper triangle of the entry pairs only: tiles from the block's own onward, in its own tile the entries behind the lane's; the
// group test (no memory, no arithmetic to speak of) stands in front of the distance test.
__global__ __launch_bounds__(256) void k_contact_brute(vmd_contact_brute_params_t p) {
    __shared__ float s_r[3][256];
    __shared__ uint32_t s_g[256];
    if (p.skip && *p.skip) return;
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const float* fx = p.xyz + (size_t)b * p.frame_stride;
    const float* fy = fx + p.row_stride;
    const float* fz = fy + p.row_stride;
    const vmd_box_t bx = vmd_load_box(p.boxes, b, p.pbc);
    const bool valid = t < p.nent;
    const uint32_t* canon = p.canon + (size_t)b * p.nent;
    float xi = VMD_FAR, yi = VMD_FAR, zi = VMD_FAR;
    uint32_t gl = 0;
    if (valid) {
        const int a = p.ent[t];
        vmd_pair_coords(bx, fx[a], fy[a], fz[a], xi, yi, zi);
        gl = (uint32_t)p.grp[canon[t]];
    }
    uint32_t* row = p.bits + (size_t)b * p.W;
    const uint32_t G = p.ngroups, min_sep = p.min_sep;
    vmd_all_pairs<256>(s_r, bx, fx, fy, fz, p.ent, p.nent, blockIdx.x * 256, valid, xi, yi, zi,
        [&](int jj, int pos) { s_g[jj] = (uint32_t)p.grp[canon[pos]]; },
        [&](int jj, int pos, float ex, float ey, float ez) {
            if (pos <= t) return false;
            const uint32_t go = s_g[jj];
            if ((go > gl ? go - gl : gl - go) >= min_sep && vmd_within_hit(p.w, vmd_d2(ex, ey, ez))) vmd_contact_hit(row, G, min_sep, gl, go);
            return false;
        });
}

// The finish, behind the walk or all pairs over a frame group: three launches under the overflow flag.
struct vmd_contact_finish_params_t {
    const uint32_t* bits; uint32_t W, P; int B;
    const uint32_t* native; int nnative;       // the native pairs' condensed indices
    unsigned* counts;                           // u32[2 B], zeroed by the launcher: the pairs, the native pairs in contact per frame
    float* out_count; float* out_q; uint64_t* acc; const uint32_t* skip;
};
// one lane per WORD of the rows, read once per frame, coalesced: the lane counts its 32 pairs at once in 16 bit planes (a carry-save
// add of the frame's word into c[0 .. 15]: plane k holds bit k of all 32 counts; B <= 65535 frames fit), then adds every nonzero count
// to its record row.  The 32 rows belong to this lane of this launch alone - a frame group's partial is added to by the launches of one
// stream, one after the other - so the add is a plain one, as k_hbond_finish's of the frames row.
__global__ __launch_bounds__(256) void k_contact_finish_rows(vmd_contact_finish_params_t q) {
    if (q.skip && *q.skip) return;
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= q.W) return;
    uint32_t c[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) c[k] = 0u;
    const uint32_t* col = q.bits + w;
    for (int b = 0; b < q.B; ++b) {
        uint32_t carry = col[(size_t)b * q.W];
#pragma unroll
        for (int k = 0; k < 16; ++k) { const uint32_t t = c[k] & carry; c[k] ^= carry; carry = t; }
    }
    uint32_t any = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) any |= c[k];
    for (uint32_t i = 0; i < 32u && any; ++i) {
        if (!((any >> i) & 1u)) continue;
        uint32_t sum = 0u;
#pragma unroll
        for (int k = 0; k < 16; ++k) sum |= ((c[k] >> i) & 1u) << k;
        const uint32_t p = 32u * w + i;
        if (p < q.P) q.acc[p] += (uint64_t)sum;
    }
}
// grid.y = the frame.  Blocks x < ceil(W / 256): one lane per word, the popcount of the row (a row's last word holds no bit beyond P: only
// pair indices are ever set), reduced over the wave into one u32 atomic; the blocks behind them: one lane per native pair, its bit likewise.
__global__ __launch_bounds__(256) void k_contact_finish_frames(vmd_contact_finish_params_t q) {
    if (q.skip && *q.skip) return;
    const int b = blockIdx.y;
    const uint32_t* row = q.bits + (size_t)b * q.W;
    const uint32_t wblocks = (q.W + 255u) / 256u;
    if (blockIdx.x < wblocks) {
        const uint32_t i = blockIdx.x * 256u + threadIdx.x;
        uint32_t v = i < q.W ? row[i] : 0u;
        if (i + 1 == q.W && (q.P & 31u)) v &= (1u << (q.P & 31u)) - 1u;
        vmd_wave_add_u32(q.counts + b, vmd_popc_u32(v));
    } else {
        const uint32_t i = (blockIdx.x - wblocks) * 256u + threadIdx.x;
        unsigned n = 0;
        if (i < (uint32_t)q.nnative) { const uint32_t p = q.native[i]; n = (row[p >> 5] >> (p & 31u)) & 1u; }
        vmd_wave_add_u32(q.counts + q.B + b, n);
    }
}
// the temporal rows - Q = (float)n / (float)nnative, one fp32 division - and the frames row, bumped once per frame
__global__ __launch_bounds__(256) void k_contact_finish_out(vmd_contact_finish_params_t q) {
    if (q.skip && *q.skip) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < q.B) {
        q.out_count[i] = (float)q.counts[i];
        if (q.out_q) q.out_q[i] = (float)q.counts[q.B + i] / (float)q.nnative;
    }
    if (i == 0) q.acc[q.P] += (uint64_t)q.B;
}

// ------------------------------------------------------------------------------------------------ K15: clusters of groups

// One list of entries (atom, group) against itself, as K14's.  Groups g != h are BONDED in a frame when an entry of g and an entry of h pass
// within()'s pair distance (rule 1 of K12, word for word; no min_sep); the clusters of the frame are the connected components of that graph
// over all G groups.  DECISION(D-CL-GEOMETRIC): the lane of an entry takes its group from the LIST, a hit takes its group through the
// identity table (the lowest entry coinciding with the slot).  Coincident entries stand at distance 0 of each other, so their groups are
// bonded, and whichever of them a third entry is said to have met, the closure is the same: the components are the geometric ones and no
// coincidence rule enters into them (no vmd_own_slots search in the walk, no k_canon_entries pass in front of all pairs).
//
// The components are made by a concurrent union-find over the hits, on the frame's row of `parent`, u32[B][G], preset to parent[g] = g.
// A root is hooked under a LOWER root only, with one compare-and-swap; so a non-root's parent is always lower than itself, a word only
// ever decreases, and the final root of a component is its lowest group whatever the order of the hits - its label.  No lane ever waits
// for another: a failed compare-and-swap proves that another lane's hook of the same root succeeded, a root is hooked once, at most G - 1
// hooks succeed per frame, and a find walks strictly downwards; so every loop is bounded and there is no spin, no lock and no flag.
// Inside the launch EVERY read and write of a parent word is an agent-scope atomic - relaxed loads, atomicCAS for the hook, atomicMin for
// path halving: a plain load may be served from a CU's L1 that no other CU's store refreshes, and a retry loop fed by it need not end.
// (The SIMT emulator runs one lane at a time and its header has none of the three: there they are the plain forms, as vmd_atomic_min_u32's.)
__device__ __forceinline__ uint32_t vmd_atomic_load_u32(uint32_t* p) {
#ifdef __HIPCC__
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}
__device__ __forceinline__ uint32_t vmd_atomic_cas_u32(uint32_t* p, uint32_t expected, uint32_t v) {
#ifdef __HIPCC__
    return atomicCAS(p, expected, v);
#else
    const uint32_t old = *p;
    if (old == expected) *p = v;
    return old;
#endif
}
// the root of g's tree as some moment of the launch saw it; path halving on the way (parent[g] <- an ancestor, which is lower: atomicMin)
__device__ __forceinline__ uint32_t vmd_cluster_find(uint32_t* parent, uint32_t g) {
    for (;;) {
        const uint32_t p = vmd_atomic_load_u32(parent + g);
        if (p == g) return g;
        const uint32_t gp = vmd_atomic_load_u32(parent + p);
        if (gp != p) vmd_atomic_min_u32(parent + g, gp);
        g = gp;                          // (gp <= p < g: strictly downwards)
    }
}
// a and b into one tree -> its root as this lane left it (the lower of the two roots)
__device__ __forceinline__ uint32_t vmd_cluster_union(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = vmd_cluster_find(parent, a);
        b = vmd_cluster_find(parent, b);
        if (a == b) return a;
        const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
        const uint32_t old = vmd_atomic_cas_u32(parent + hi, hi, lo);
        if (old == hi) return lo;
        a = old; b = lo;                 // another lane hooked hi first: again from what it hooked it under
    }
}

struct vmd_cluster_atoms_params_t {
    vmd_cells_params_t c;       // the entries as their cell build read them: raw frame, the GRID's boxes, pbc, the list, grid (no outputs)
    vmd_within_walk_params_t k; // the cell-sorted copy of the SAME list, the test of within(r_cut, .)
    const int32_t* grp; uint32_t ngroups;
    const uint32_t* ident;      // k_sorted_atoms' table of the copy, u32[B][k.nref_pad]
    uint32_t* parent;           // u32[B][ngroups], preset by k_cluster_init
    const uint32_t* skip;
};

// parent[b][g] = g in front of every walk and every all pairs, a repeated batch included
__global__ __launch_bounds__(256) void k_cluster_init(uint32_t* parent, uint32_t G, const uint32_t* skip) {
    if (skip && *skip) return;
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < G) parent[(size_t)blockIdx.y * G + g] = g;
}

// The walk, one lane per entry in list order, standing where vmd_walk_lane puts it, its group from the list.  Every hit of another group
// is a union.  SKIP (option cluster_skip_same, measured and off by default): the lane keeps the last group it joined and the
// root that union left - a member of its own tree, so the next union may start from it - and skips the hits that repeat that group.
template <bool SKIP>
__global__ __launch_bounds__(256) void k_cluster_atoms(vmd_cluster_atoms_params_t p) {
    if (p.skip && *p.skip) return;       // a cell build of this batch overflowed a bucket: the table and the copy are void
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.c.nsel) return;
    const vmd_within_walk_t k = vmd_within_walk_setup(p.c.boxes, b, p.c.pbc, p.c.grid, p.k);
    const uint32_t* id = p.ident + (size_t)b * p.k.nref_pad;
    const uint32_t n = (uint32_t)p.c.nsel;
    const int32_t* grp = p.grp;
    uint32_t* parent = p.parent + (size_t)b * p.ngroups;
    const vmd_walk_lane_t l = vmd_walk_lane(p.c, k, b, t);
    const uint32_t gl = (uint32_t)grp[t];
    uint32_t mine = gl, last = gl;
    vmd_within_walk_each(k, l.py, l.pz, l.x, l.y, l.z, [&](unsigned j, float, float, float) {
        const uint32_t a = id[j];
        if (a >= n) return false;        // (an unclaimed slot would be a bug of k_sorted_atoms; it is never an index)
        const uint32_t go = (uint32_t)grp[a];
        if (go == gl || (SKIP && go == last)) return false;
        const uint32_t r = vmd_cluster_union(parent, mine, go);
        if (SKIP) { mine = r; last = go; }
        return false;
    });
}

struct vmd_cluster_brute_params_t {
    const float* xyz; size_t frame_stride; size_t row_stride;
    const float* boxes; uint32_t pbc;
    const int32_t* ent; const int32_t* grp; int nent; uint32_t ngroups;
    vmd_within_test_t w;        // within(r_cut, .)
    uint32_t* parent; const uint32_t* skip;
};

// All pairs from the raw frame: one lane per entry over vmd_all_pairs, the list staged with every entry's group from the list.  The upper
// triangle of the entry pairs only, as k_contact_brute's; the group test stands in front of the distance test.  The same union.
__global__ __launch_bounds__(256) void k_cluster_brute(vmd_cluster_brute_params_t p) {
    __shared__ float s_r[3][256];
    __shared__ uint32_t s_g[256];
    if (p.skip && *p.skip) return;
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const float* fx = p.xyz + (size_t)b * p.frame_stride;
    const float* fy = fx + p.row_stride;
    const float* fz = fy + p.row_stride;
    const vmd_box_t bx = vmd_load_box(p.boxes, b, p.pbc);
    const bool valid = t < p.nent;
    float xi = VMD_FAR, yi = VMD_FAR, zi = VMD_FAR;
    uint32_t gl = 0;
    if (valid) {
        const int a = p.ent[t];
        vmd_pair_coords(bx, fx[a], fy[a], fz[a], xi, yi, zi);
        gl = (uint32_t)p.grp[t];
    }
    uint32_t* parent = p.parent + (size_t)b * p.ngroups;
    vmd_all_pairs<256>(s_r, bx, fx, fy, fz, p.ent, p.nent, blockIdx.x * 256, valid, xi, yi, zi,
        [&](int jj, int pos) { s_g[jj] = (uint32_t)p.grp[pos]; },
        [&](int jj, int pos, float ex, float ey, float ez) {
            if (pos <= t) return false;
            const uint32_t go = s_g[jj];
            if (go != gl && vmd_within_hit(p.w, vmd_d2(ex, ey, ez))) vmd_cluster_union(parent, gl, go);
            return false;
        });
}

// The finish, behind the walk or all pairs over a frame group: three launches under the overflow flag.  They stand behind a kernel
// boundary, so the parent words are read with plain loads here.
struct vmd_cluster_finish_params_t {
    const uint32_t* parent; uint32_t* root; uint32_t* size; uint32_t G; int B;
    unsigned* counts;                           // u32[2 B], zeroed by the launcher: the clusters, the largest cluster per frame
    float* out_count; float* out_largest; uint64_t* acc; const uint32_t* skip;      // (the three may be NULL: the labels of one frame)
};
// one lane per (frame, group): the group's root - its label, what vmd_eval_cluster_labels copies back - and one count into the root's size
__global__ __launch_bounds__(256) void k_cluster_finish_roots(vmd_cluster_finish_params_t q) {
    if (q.skip && *q.skip) return;
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= q.G) return;
    const size_t row = (size_t)blockIdx.y * q.G;
    const uint32_t* parent = q.parent + row;
    uint32_t r = g;
    for (uint32_t p = parent[r]; p < r; p = parent[r]) r = p;          // (p < r or p == r: a walk strictly downwards, whatever the words hold)
    q.root[row + g] = r;
    atomicAdd(q.size + row + r, 1u);
}
// one lane per (frame, group), acting where the group is a root: the clusters of the frame summed over the wave, the largest by atomicMax,
// one u64 add into row size - 1 of the record's partial.  SINGLES (option cluster_wave_singles, measured and kept): the clusters of ONE group - in a dilute system
// nearly every lane - are summed over the wave into one add to row 0.
template <bool SINGLES>
__global__ __launch_bounds__(256) void k_cluster_finish_count(vmd_cluster_finish_params_t q) {
    if (q.skip && *q.skip) return;
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    const int b = blockIdx.y;
    const size_t row = (size_t)b * q.G;
    const bool is_root = g < q.G && q.root[row + g] == g;
    const uint32_t s = is_root ? q.size[row + g] : 0u;
    vmd_wave_add_u32(q.counts + b, is_root ? 1u : 0u);
    if (is_root) atomicMax(q.counts + q.B + b, s);
    if (!q.acc) return;
    if (SINGLES) vmd_wave_add_u64(q.acc, s == 1u ? 1u : 0u);
    if (s > (SINGLES ? 1u : 0u)) vmd_atomic_add_u64(q.acc + (s - 1u), 1u);
}
// the temporal rows and the frames row, bumped once per frame
__global__ __launch_bounds__(256) void k_cluster_finish_out(vmd_cluster_finish_params_t q) {
    if (q.skip && *q.skip) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < q.B) {
        if (q.out_count) q.out_count[i] = (float)q.counts[i];
        if (q.out_largest) q.out_largest[i] = (float)q.counts[q.B + i];
    }
    if (i == 0 && q.acc) q.acc[q.G] += (uint64_t)q.B;
}

// ------------------------------------------------------------------------------------------------ K16: mean-squared displacement

// The position table: row f = x[n], y[n], z[n] of the listed atoms as the frame holds them, then the frame's cell as every kernel reads it
// ({L, 1/L, tilts}, VMD_BOX_STRIDE floats) with L = 1/L = 0 on an axis that is not periodic (its flag is clear, or THIS frame's edge is
// not positive - whatever frame leads the batch), so that the table says by itself which axes
// the unwrap follows.  One lane per (frame, entry of a row), the entry fastest: the reads of the cell and the writes are coalesced, the
// gathers follow the list.  Nothing is computed.
struct vmd_msd_gather_params_t {
    vmd_frames_t f;
    const int32_t* idx; int n;
    float* rows;   // [B][3 n + 9]
};
__global__ __launch_bounds__(256) void k_msd_gather(vmd_msd_gather_params_t p) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int w = 3 * p.n + VMD_BOX_STRIDE;
    if (j >= w) return;
    float v;
    if (j < 3 * p.n) {
        const int k = j / p.n, i = j - k * p.n;
        v = p.f.xyz[(size_t)b * p.f.frame_stride + (size_t)k * p.f.row_stride + (size_t)p.idx[i]];
    } else {
        const int c = j - 3 * p.n;
        v = p.f.boxes[(size_t)VMD_BOX_STRIDE * b + c];
        if (c < 6 && !(((p.f.pbc >> (c % 3)) & 1u) && p.f.boxes[(size_t)VMD_BOX_STRIDE * b + c % 3] > 0.0f)) v = 0.0f;     // the frame's own edge, not the batch's
    }
    p.rows[(size_t)b * w + j] = v;
}

// DECISION(D-MSD-UNWRAP): the image counts of the window, exact, in integers.  One lane per atom walks frames 0 .. F - 1 of the window in
// order; per axis the count stands at 0 in frame 0 and, from t to t + 1, the SPEC S3 rule (vmd_mi_cmp's comparisons) under the cell of frame
// t + 1 decides: a difference above half a cell took one cell too many, the count goes down by one; below minus half a cell, up by one; a
// difference of exactly half a cell is no crossing (S3's tie).  x + count * L is then the unwrapped coordinate.  An axis with L = 0 in frame
// t + 1 keeps its count.  counts: i32[F][3][n], one word per axis (the range of a count is that of an int).
struct vmd_msd_unwrap_params_t {
    const float* rows; int F; int n;
    int* counts;
};
__global__ __launch_bounds__(256) void k_msd_unwrap(vmd_msd_unwrap_params_t p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const size_t w = 3 * (size_t)p.n + VMD_BOX_STRIDE, cw = 3 * (size_t)p.n;
    int c[3] = {0, 0, 0};
    float prev[3];
    for (int k = 0; k < 3; ++k) { prev[k] = p.rows[(size_t)k * p.n + i]; p.counts[(size_t)k * p.n + i] = 0; }
    for (int t = 1; t < p.F; ++t) {
        const float* row = p.rows + (size_t)t * w;
        for (int k = 0; k < 3; ++k) {
            const float x = row[(size_t)k * p.n + i], L = row[3 * (size_t)p.n + k];
            if (L > 0.0f) {
                const float d = x - prev[k], hL = 0.5f * L;
                c[k] += d > hL ? -1 : (d < -hL ? 1 : 0);
            }
            prev[k] = x;
            p.counts[(size_t)t * cw + (size_t)k * p.n + i] = c[k];
        }
    }
}

// The sums over origins and atoms, one lane per LAG.  A block takes a tile of VMD_MSD_A atoms, a span of VMD_MSD_SO origin frames and a chunk
// of VMD_MSD_LC lags (its threads), and stages what they touch into LDS laid out [atom][axis][frame]: the origins' frames [s0, s0 + SO) and
// the targets' frames [s0 + l0, s0 + l0 + SO + LC - 1) - positions, image counts and, once per frame, the cell's edges.  Lane `tid` holds lag
// l0 + tid: for origin s0 + i its target sits at entry i + tid of the target rows, so the 64 lanes of a wave read 64 consecutive words (no
// bank conflict) and the origin's own values are one word for all of them (a broadcast).  The displacement is formed as DESIGN 1.18 states it,
// every operation rounded on its own (this file is compiled without contraction), and every term is an integer before it is summed: the
// sums do not depend on the order of lanes, blocks or atomics.  A block walks the atom tiles blockIdx.x, blockIdx.x + gridDim.x, ... with its
// four u64 sums in registers and ends with four 64-bit atomics per lag.  A lane whose lag lies beyond max_lag, an origin off the stride or
// beyond the window and a target beyond the window do nothing.
#define VMD_MSD_A 8
#define VMD_MSD_SO 32
#define VMD_MSD_LC 256
#define VMD_MSD_FT (VMD_MSD_SO + VMD_MSD_LC - 1)
struct vmd_msd_lags_params_t {
    const float* rows; const int* counts;      // the window's rows of the table, its image counts
    int F; int n; int max_lag; int stride;
    unsigned long long* sums;                   // [max_lag + 1][4]
};
__global__ __launch_bounds__(VMD_MSD_LC) void k_msd_lags(vmd_msd_lags_params_t p) {
    __shared__ float s_ox[VMD_MSD_A][3][VMD_MSD_SO];
    __shared__ int s_on[VMD_MSD_A][3][VMD_MSD_SO];
    __shared__ float s_tx[VMD_MSD_A][3][VMD_MSD_FT];
    __shared__ int s_tn[VMD_MSD_A][3][VMD_MSD_FT];
    __shared__ float s_L[3][VMD_MSD_FT];
    const int tid = threadIdx.x;
    const int s0 = (int)blockIdx.y * VMD_MSD_SO, l0 = (int)blockIdx.z * VMD_MSD_LC;
    const int t0 = s0 + l0;                                     // the first target frame
    if (t0 >= p.F) return;                                      // (the whole block: no origin of the span has a target in the window)
    const int lag = l0 + tid;
    const size_t w = 3 * (size_t)p.n + VMD_BOX_STRIDE, cw = 3 * (size_t)p.n;
    const int no = p.F - s0 < VMD_MSD_SO ? p.F - s0 : VMD_MSD_SO, nt = p.F - t0 < VMD_MSD_FT ? p.F - t0 : VMD_MSD_FT;
    for (int j = tid; j < 3 * VMD_MSD_FT; j += VMD_MSD_LC) {
        const int k = j / VMD_MSD_FT, f = j - k * VMD_MSD_FT;
        s_L[k][f] = f < nt ? p.rows[(size_t)(t0 + f) * w + 3 * (size_t)p.n + k] : 0.0f;
    }
    // the origins of the span this lane has a term for: on the stride, and with the target inside the window
    const int ntiles = (p.n + VMD_MSD_A - 1) / VMD_MSD_A;
    unsigned long long acc[4] = {0ull, 0ull, 0ull, 0ull};
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int a0 = tile * VMD_MSD_A, na = p.n - a0 < VMD_MSD_A ? p.n - a0 : VMD_MSD_A;
        __syncthreads();                                        // the previous tile has been read (and s_L written)
        for (int j = tid; j < VMD_MSD_A * 3 * VMD_MSD_SO; j += VMD_MSD_LC) {
            const int a = j % VMD_MSD_A, r = j / VMD_MSD_A, k = r % 3, f = r / 3;
            const bool in = a < na && f < no;
            s_ox[a][k][f] = in ? p.rows[(size_t)(s0 + f) * w + (size_t)k * p.n + (size_t)(a0 + a)] : 0.0f;
            s_on[a][k][f] = in ? p.counts[(size_t)(s0 + f) * cw + (size_t)k * p.n + (size_t)(a0 + a)] : 0;
        }
        for (int j = tid; j < VMD_MSD_A * 3 * VMD_MSD_FT; j += VMD_MSD_LC) {
            const int a = j % VMD_MSD_A, r = j / VMD_MSD_A, k = r % 3, f = r / 3;
            const bool in = a < na && f < nt;
            s_tx[a][k][f] = in ? p.rows[(size_t)(t0 + f) * w + (size_t)k * p.n + (size_t)(a0 + a)] : 0.0f;
            s_tn[a][k][f] = in ? p.counts[(size_t)(t0 + f) * cw + (size_t)k * p.n + (size_t)(a0 + a)] : 0;
        }
        __syncthreads();
        if (lag > p.max_lag) continue;                          // (it still meets the barriers above)
        for (int i = 0; i < no; ++i) {
            const int t = s0 + i;
            if (t % p.stride != 0 || t + lag >= p.F) continue;
            const int f = i + tid;                              // < FT, and < nt: t0 + f = t + lag < F
            const float Lx = s_L[0][f], Ly = s_L[1][f], Lz = s_L[2][f];
            auto term = [&](int a) {
                const float dx = (s_tx[a][0][f] - s_ox[a][0][i]) + (float)(s_tn[a][0][f] - s_on[a][0][i]) * Lx;
                const float dy = (s_tx[a][1][f] - s_ox[a][1][i]) + (float)(s_tn[a][1][f] - s_on[a][1][i]) * Ly;
                const float dz = (s_tx[a][2][f] - s_ox[a][2][i]) + (float)(s_tn[a][2][f] - s_on[a][2][i]) * Lz;
                acc[0] += (unsigned long long)((dx * dx) * 1048576.0f);
                acc[1] += (unsigned long long)((dy * dy) * 1048576.0f);
                acc[2] += (unsigned long long)((dz * dz) * 1048576.0f);
            };
            if (na == VMD_MSD_A) {                              // a whole tile: unrolled, its reads in flight together
#pragma unroll
                for (int a = 0; a < VMD_MSD_A; ++a) term(a);
            } else for (int a = 0; a < na; ++a) term(a);
            acc[3] += (unsigned long long)na;
        }
    }
    if (lag > p.max_lag || !acc[3]) return;
    for (int k = 0; k < 4; ++k) atomicAdd(&p.sums[4 * (size_t)lag + k], acc[k]);
}

// ------------------------------------------------------------------------------------------------ misc

__global__ __launch_bounds__(256) void k_counts_to_float(const uint64_t* __restrict__ counts, size_t n, float* __restrict__ values,
                                                         unsigned* __restrict__ max_bits, float scale) {
    // 8 voxels per thread, one atomicMax per WAVE: a filled 128^3 volume used to issue ~10^6 same-address atomics (0.38 ms per call,
    // more than the conversion's 25 MB of traffic costs)
    const size_t i0 = (size_t)blockIdx.x * 2048 + threadIdx.x;
    float vmax = 0.0f;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const size_t i = i0 + 256 * (size_t)u;
        if (i < n) { const float v = (float)counts[i] * scale; values[i] = v; vmax = fmaxf(vmax, v); }   // scale = 1: raw counts (SPEC S5)
    }
    if (max_bits) {
        vmax = vmd_wave_max(vmax);
        if ((threadIdx.x & 63) == 0 && vmax > 0.0f) atomicMax(max_bits, (unsigned)__float_as_int(vmax));
    }
}

__device__ __forceinline__ uint64_t vmd_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ float vmd_synth_uniform(uint64_t seed, uint32_t stream, uint32_t frame, uint32_t atom) {
    const uint64_t key = vmd_mix64(seed * 0x9E3779B97F4A7C15ull + (uint64_t)stream);
    const uint64_t h = vmd_mix64(key ^ (((uint64_t)frame << 32) | (uint64_t)atom));
    return (float)(uint32_t)(h >> 40) * (1.0f / 16777216.0f);
}

struct vmd_synth_params_t {
    float* xyz; size_t frame_stride; size_t row_stride; int B; uint32_t frame0;
    uint64_t seed; uint32_t n_atoms; uint32_t n_blob; float L; float sigma;
};

// oracle S9 twin: integer RNG, explicit rounding steps -> bit-identical to vo_synth_frame
__global__ __launch_bounds__(256) void k_synth(vmd_synth_params_t p) {
    const uint32_t i = p.n_blob + blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= p.n_atoms) return;
    const uint32_t frame = p.frame0 + (uint32_t)b;
    const float sig = (float)((double)p.sigma * sqrt((double)frame));
    const uint32_t w = i - p.n_blob;
    const uint32_t mol = w / 3u, site = w % 3u;
    float* f = p.xyz + (size_t)b * p.frame_stride;
    for (uint32_t c = 0; c < 3; ++c) {
        float p0 = vmd_synth_uniform(p.seed, 1u + c, 0u, mol) * p.L;
        if (site) {
            const float off = (vmd_synth_uniform(p.seed, 4u + 3u * (site - 1u) + c, 0u, mol) - 0.5f) * 1.1f;
            p0 = p0 + off;
        }
        const float g = (((vmd_synth_uniform(p.seed, 10u + c, frame, i) + vmd_synth_uniform(p.seed, 13u + c, frame, i)) +
                          (vmd_synth_uniform(p.seed, 16u + c, frame, i) + vmd_synth_uniform(p.seed, 19u + c, frame, i))) - 2.0f) * 1.7320508f;
        const float t = sig * g;
        f[(size_t)c * p.row_stride + i] = vmd_wrap(p0 + t, p.L, 1.0f / p.L);
    }
}

// ================================================================================================ C ABI

#define VMD_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

static int g_cells_fused = 1;
extern "C" int vmd_hip_set_cells_fused(int on) { const int old = g_cells_fused; g_cells_fused = on; return old; }
static int g_cells_split = 1;
extern "C" int vmd_hip_set_cells_split(int on) { const int old = g_cells_split; g_cells_split = on; return old; }
// the fused single-block-per-frame build needs the cell table in LDS (<= 96 KB of counters)
// ... and pays off while one block per frame still has enough parallelism (measured: 33k atoms/frame 1.5x faster, 333k slower)
extern "C" int vmd_hip_cells_fused_ok(vmd_grid_t grid, int nsel) { return g_cells_fused && g_cells_split < 2 && grid.ncell + 1 <= 24576 && nsel <= 65536; }
// larger selections: G blocks per frame with LDS tables (k_cells_split_*); 0 = not applicable
// (cells_split = 2 forces this path with 2048-atom slices whatever the selection size, >= 1024 forces it with that slice
// size: test / tuning hook)
static int vmd_split_slice(void) { return g_cells_split == 2 ? 2048 : g_cells_split >= 1024 ? (g_cells_split & ~1023) : 32768; }
extern "C" int vmd_hip_cells_split_blocks(vmd_grid_t grid, int nsel) {
    if (!g_cells_fused || !g_cells_split || grid.ncell + 1 > 24576 || (nsel <= 65536 && g_cells_split < 2)) return 0;
    return (nsel + vmd_split_slice() - 1) / vmd_split_slice();
}
// u32 words of `rank` scratch per frame that vmd_hip_cells_build needs for this grid and selection
extern "C" size_t vmd_hip_cells_scratch_words(vmd_grid_t grid, int nsel) {
    const size_t split = (size_t)vmd_hip_cells_split_blocks(grid, nsel) * (size_t)grid.ncell;
    return split > (size_t)nsel ? split : (size_t)nsel;
}

#define VMD_LDS_OPT_IN (160 * 1024 - 64)     // bytes of dynamic LDS the kernels of this file opt in to, and the limit its launch code sizes tables against
static int vmd_lds_opt_in(const void* kernel) {
    return (int)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, VMD_LDS_OPT_IN);
}

// per host thread, set by the evaluator before the builds of one selection and cleared after them (like the overflow bit below): the
// periodic form of that selection's index list, or m = 0
static thread_local vmd_sel_pattern_t g_cells_sel_pattern = {0, 0, 0, {0, 0, 0, 0}};
extern "C" void vmd_hip_set_cells_sel_pattern(int m, int first, int period, const int* off) {
    vmd_sel_pattern_t p = {0, 0, 0, {0, 0, 0, 0}};
    if (m >= 1 && m <= 4 && period > 0) {
        p.m = m; p.first = first; p.period = period;
        for (int k = 0; k < m; ++k) p.off[k] = off ? off[k] : 0;
    }
    g_cells_sel_pattern = p;
}
// what every build kernel is told about the frames, the selection (the thread's pattern included) and the grid; the outputs and the scratch
// of the single-level builds are the caller's to add
static vmd_cells_params_t vmd_cells_params(const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags,
                                           const int32_t* sel, int nsel, int nsel_pad, vmd_grid_t grid) {
    vmd_cells_params_t p = {};
    p.xyz = xyz; p.frame_stride = frame_stride; p.row_stride = row_stride; p.boxes = boxes; p.pbc = pbc_flags;
    p.sel = sel; p.nsel = nsel; p.nsel_pad = nsel_pad; p.grid = grid; p.pat = g_cells_sel_pattern;
    return p;
}

extern "C" int vmd_hip_cells_build(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                                   const float* boxes, uint32_t pbc_flags, int B, const int32_t* sel, int nsel, int nsel_pad,
                                   vmd_grid_t grid, uint32_t* cell_count, uint32_t* rank, uint32_t* cell_start, float* sorted,
                                   float* aos) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0 || nsel <= 0) return 0;
    const dim3 grp((nsel + 255) / 256, B);
    vmd_cells_params_t p = vmd_cells_params(xyz, frame_stride, row_stride, boxes, pbc_flags, sel, nsel, nsel_pad, grid);
    p.cell_count = cell_count; p.rank = rank; p.cell_start = cell_start; p.sorted = sorted; p.aos = aos;
    if (vmd_hip_cells_fused_ok(grid, nsel)) {
        const size_t shm = sizeof(uint32_t) * ((size_t)grid.ncell + 1 + 1024);
        int ea = vmd_lds_opt_in((const void*)k_cells_fused);
        if (ea) return ea;
        hipLaunchKernelGGL(k_cells_fused, dim3(B), dim3(1024), shm, s, p);
        VMD_LAUNCH_CHECK();
    } else if (const int G = vmd_hip_cells_split_blocks(grid, nsel)) {
        vmd_cells_split_t q{p, rank, G, vmd_split_slice()};
        const size_t shm = sizeof(uint32_t) * (size_t)grid.ncell;
        int ea = vmd_lds_opt_in((const void*)k_cells_split_count);
        if (!ea) ea = vmd_lds_opt_in((const void*)k_cells_split_scatter);
        if (ea) return ea;
        hipLaunchKernelGGL(k_cells_split_count, dim3(G, B), dim3(1024), shm, s, q);
        VMD_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_cells_split_scan, dim3(B), dim3(1024), 0, s, rank, cell_start, (int)grid.ncell, G);
        VMD_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_cells_split_scatter, dim3(G, B), dim3(1024), shm, s, q);
        VMD_LAUNCH_CHECK();
    } else {
        hipError_t e = hipMemsetAsync(cell_count, 0, sizeof(uint32_t) * (size_t)B * (grid.ncell + 1), s);
        if (e != hipSuccess) return (int)e;
        const dim3 g((nsel + 256 * VMD_CELLS_ILP - 1) / (256 * VMD_CELLS_ILP), B);
        hipLaunchKernelGGL(k_cells_count, g, dim3(256), 0, s, p);
        VMD_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_cells_scan, dim3(B), dim3(1024), 0, s, (const uint32_t*)cell_count, cell_start, (int)grid.ncell);
        VMD_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_cells_scatter, g, dim3(256), 0, s, p);
        VMD_LAUNCH_CHECK();
    }
    if (aos) { hipLaunchKernelGGL(k_cells_repack, grp, dim3(256), 0, s, (const float*)aos, sorted, nsel, nsel_pad); VMD_LAUNCH_CHECK(); }
    return 0;
}

// which pop the hit stack of k_rdf_pencil (variant 0) is drained with when r_min == 0: 0 = vmd_pop_hot (9 VALU instructions), 1 = vmd_pop_hot0
// (delta folded into the constant, a spare bin instead of the range compare, the stack read with ds_read_addtid_b32: 6).  A/B and cross-check
// switch; measured on c3: 73.3 -> 71.9 ms per 1 000 frames (profiles/r06q_pop_compile_time_ab.txt; the variant with a plain ds_read, 7
// instructions, sits between them: profiles/r06p_pop_ab.txt)
static int g_rdf_pop = 1;
extern "C" int vmd_hip_set_rdf_pop(int mode) { const int old = g_rdf_pop; if (mode >= 0 && mode <= 1) g_rdf_pop = mode; return old; }
static int g_rdf_nsub = 0;   // 0 = automatic: about one i-chunk per item
extern "C" int vmd_hip_set_rdf_nsub(int n) { const int old = g_rdf_nsub; if (n >= 0 && n <= 64) g_rdf_nsub = n; return old; }
static int g_rdf_nsub_pct = 100;   // automatic nsub = mean chunks per pencil x this / 100
extern "C" int vmd_hip_set_rdf_nsub_pct(int n) { const int old = g_rdf_nsub_pct; if (n >= 25 && n <= 800) g_rdf_nsub_pct = n; return old; }
static int g_rdf_shist = 1;       // one LDS histogram per block instead of one per wave: 8 instead of 7 waves per SIMD (default since round 6, see VMD_PENCIL_OCC)
extern "C" int vmd_hip_set_rdf_shared_hist(int on) { const int old = g_rdf_shist; g_rdf_shist = on ? 1 : 0; return old; }
// an image segment whose shift has one live axis subtracts that one only (vmd_segment); 0 = every shifted segment takes the general loop.  A/B and
// cross-check switch: the counts are the same bit for bit (tests/pencil_loop_cases.py), measured in profiles/pair_loops_ab.txt
static int g_rdf_shift_axes = 1;
extern "C" int vmd_hip_set_rdf_shift_axes(int on) { const int old = g_rdf_shift_axes; g_rdf_shift_axes = on ? 1 : 0; return old; }
static thread_local int g_pen_ry = 1, g_pen_rz = 1;   // neighbour reach of the pencil walk; the grid handed to the build and to the walk must be cut to match.  Per host thread like g_rdf_closed: the evaluator sets it (choose_grid) right before that thread's launches, two evals on two threads must not race (TSan: profiles/r04r_tsan.txt)
extern "C" void vmd_hip_set_pencil_reach(int ry, int rz) { g_pen_ry = ry < 1 ? 1 : (ry > 4 ? 4 : ry); g_pen_rz = rz < 1 ? 1 : (rz > 4 ? 4 : rz); }
// candidate columns walked by k_rdf_pencil (all launches of this process on the current device) since the last reset
static unsigned long long* g_cols_dev[64] = {};
static unsigned long long* vmd_cols_counter() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (!g_cols_dev[dev]) {
        if (hipMalloc((void**)&g_cols_dev[dev], sizeof(unsigned long long)) != hipSuccess) { g_cols_dev[dev] = nullptr; return nullptr; }
        (void)hipMemset(g_cols_dev[dev], 0, sizeof(unsigned long long));
    }
    return g_cols_dev[dev];
}
extern "C" uint64_t vmd_hip_rdf_columns(int reset) {
    unsigned long long* c = vmd_cols_counter();
    unsigned long long v = 0;
    if (!c || hipDeviceSynchronize() != hipSuccess || hipMemcpy(&v, c, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    if (reset) (void)hipMemset(c, 0, sizeof(v));
    return (uint64_t)v;
}
static int g_rdf_nsplit = -1;     // small launches split a chunk's neighbour pencils over work items: -1 automatic (5 / 9), 0 never, n > 0 = n parts
extern "C" int vmd_hip_set_rdf_nsplit(int n) { const int old = g_rdf_nsplit; g_rdf_nsplit = n < -1 ? -1 : (n > 25 ? 25 : n); return old; }
static int g_rdf_blocks = 2048;   // 8 blocks x 4 waves per CU: all resident with the shared histogram (7 per CU with wave-private ones)
extern "C" int vmd_hip_rdf_num_blocks(void) { return 2048; }   // capacity of the partial-row scratch
extern "C" int vmd_hip_set_rdf_blocks(int n) { const int old = g_rdf_blocks; if (n >= 8 && n <= 2048) g_rdf_blocks = n; return old; }
extern "C" size_t vmd_hip_rdf_partial_words(void) {
    return (size_t)vmd_hip_rdf_num_blocks() * VMD_MAX_BINS + 8 * VMD_COUNTER_STRIDE * sizeof(unsigned) / sizeof(uint64_t);
}

extern "C" int vmd_hip_rdf_pencil(void* stream, const float* sorted_ref, const uint32_t* cell_start_ref, int nref, int nref_pad,
                                  const float* sorted_tgt, const uint32_t* cell_start_tgt, int ntgt, int ntgt_pad,
                                  const float* boxes, int B, vmd_grid_t grid, float rmin, float rmax, int nbins,
                                  int same_set, int variant, uint32_t pbc_flags, uint64_t* partial, uint64_t* counts,
                                  const uint32_t* skip_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (nbins <= 0 || nbins > VMD_MAX_BINS) return (int)hipErrorInvalidValue;
    if (B <= 0 || nref <= 0 || ntgt <= 0) return 0;
    // the work counter lives behind the partial rows (see vmd_hip_rdf_partial_words)
    unsigned* work_counter = (unsigned*)(partial + (size_t)vmd_hip_rdf_num_blocks() * VMD_MAX_BINS);
    {
        hipError_t e = hipMemsetAsync(work_counter, 0, 8 * VMD_COUNTER_STRIDE * sizeof(unsigned), s);
        if (e != hipSuccess) return (int)e;
    }
    vmd_pair_params_t p;
    p.work_counter = work_counter;
    p.sref = sorted_ref; p.cs_ref = cell_start_ref; p.nref_pad = nref_pad;
    p.stgt = sorted_tgt; p.cs_tgt = cell_start_tgt; p.ntgt_pad = ntgt_pad;
    p.boxes = boxes; p.B = B; p.grid = grid;
    p.bin = vmd_make_binning(rmin, rmax, nbins, g_rdf_closed);
    p.r2_up = nextafterf(rmax * rmax, 3.0e38f) * 1.0001f;
    p.rpad = rmax * 1.0001f + 1.0e-4f;
    p.pop = p.bin.fast_2d < 1.0f ? g_rdf_pop : 0;       // the folded test needs r_min == 0 and a usable fast path (vmd_make_binning)
    p.partial = partial;
    p.counts = (unsigned long long*)counts;
    // items per pencil: the mean number of 64-atom i-chunks in a pencil, so that an XCD's waves in flight cover as few frames
    // as possible (profiles/r01t_ab.txt: c2 +11 %, c3 +8.5 % over whole-pencil items)
    p.nsub = g_rdf_nsub;
    if (p.nsub == 0) {
        const long long per_chunk = (long long)grid.ny * grid.nz * VMD_WAVE;
        p.nsub = (int)(((nref + per_chunk - 1) / per_chunk) * g_rdf_nsub_pct / 100);
        if (p.nsub < 1) p.nsub = 1;
        if (p.nsub > 64) p.nsub = 64;
    }
    // small launches: fewer items than the grid has waves.  Every item is then a lone, latency-bound chain; dealing a chunk's neighbour
    // pencils (5 in the half shell, 9 otherwise) to separate items shortens the chains and fills the idle waves
    p.nsplit = 1;
    if (g_rdf_nsplit != 0 && (long long)B * grid.ny * grid.nz * p.nsub < 4ll * g_rdf_blocks) p.nsplit = g_rdf_nsplit > 0 ? g_rdf_nsplit : (same_set ? 5 : 9);
    const int nitems = B * grid.ny * grid.nz * p.nsub * p.nsplit;
    int nblocks = (nitems + 3) / 4;
    if (nblocks < 8) nblocks = 8;
    if (nblocks > g_rdf_blocks) nblocks = g_rdf_blocks;
    const dim3 g(nblocks), blk(256);
    p.pbc = pbc_flags;
    p.skip = skip_flag;
    p.ry = g_pen_ry; p.rz = g_pen_rz;
    p.shift_axes = g_rdf_shift_axes;
    p.cols_total = vmd_cols_counter();
    const int cell = (pbc_flags & VMD_PBC_TRICLINIC) ? 1 : ((pbc_flags & 7u) != 7u ? 2 : 0);
    const int which = (variant == 1 ? 6 : variant == 2 ? 12 : variant == 3 ? 18 : 0) + (same_set ? 3 : 0) + cell;
#define VMD_PENCIL_CASE(n, V, S, C) case n: if (g_rdf_shist) hipLaunchKernelGGL((k_rdf_pencil<V, S, C, true>), g, blk, 0, s, p); \
                                            else hipLaunchKernelGGL((k_rdf_pencil<V, S, C, false>), g, blk, 0, s, p); break;
    // variant 0 (the default): the pop is part of the instantiation (vmd_wave_acc_tt)
#define VMD_PENCIL_CASE0(n, S, C) case n: if (p.pop) { if (g_rdf_shist) hipLaunchKernelGGL((k_rdf_pencil<0, S, C, true, 2>), g, blk, 0, s, p); \
                                                       else hipLaunchKernelGGL((k_rdf_pencil<0, S, C, false, 2>), g, blk, 0, s, p); } \
                                          else if (g_rdf_shist) hipLaunchKernelGGL((k_rdf_pencil<0, S, C, true, 0>), g, blk, 0, s, p); \
                                          else hipLaunchKernelGGL((k_rdf_pencil<0, S, C, false, 0>), g, blk, 0, s, p); break;
    switch (which) {
    VMD_PENCIL_CASE0(0, false, 0) VMD_PENCIL_CASE0(1, false, 1) VMD_PENCIL_CASE0(2, false, 2)
    VMD_PENCIL_CASE0(3, true, 0) VMD_PENCIL_CASE0(4, true, 1) VMD_PENCIL_CASE0(5, true, 2)
    VMD_PENCIL_CASE(6, 1, false, 0) VMD_PENCIL_CASE(7, 1, false, 1) VMD_PENCIL_CASE(8, 1, false, 2)
    VMD_PENCIL_CASE(9, 1, true, 0) VMD_PENCIL_CASE(10, 1, true, 1) VMD_PENCIL_CASE(11, 1, true, 2)
    VMD_PENCIL_CASE(12, 2, false, 0) VMD_PENCIL_CASE(13, 2, false, 1) VMD_PENCIL_CASE(14, 2, false, 2)
    VMD_PENCIL_CASE(15, 2, true, 0) VMD_PENCIL_CASE(16, 2, true, 1) VMD_PENCIL_CASE(17, 2, true, 2)
    case 18: hipLaunchKernelGGL((k_rdf_pencil<3, false, 0, false>), g, blk, 0, s, p); break;
    case 19: hipLaunchKernelGGL((k_rdf_pencil<3, false, 1, false>), g, blk, 0, s, p); break;
    case 20: hipLaunchKernelGGL((k_rdf_pencil<3, false, 2, false>), g, blk, 0, s, p); break;
    case 21: hipLaunchKernelGGL((k_rdf_pencil<3, true, 0, false>), g, blk, 0, s, p); break;
    case 22: hipLaunchKernelGGL((k_rdf_pencil<3, true, 1, false>), g, blk, 0, s, p); break;
    case 23: hipLaunchKernelGGL((k_rdf_pencil<3, true, 2, false>), g, blk, 0, s, p); break;
    default: return (int)hipErrorInvalidValue;
    }
#undef VMD_PENCIL_CASE
#undef VMD_PENCIL_CASE0
    VMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hist_reduce, dim3((nbins + 255) / 256, (nblocks + 31) / 32), dim3(256), 0, s, (const uint64_t*)partial, nblocks, nbins, counts, skip_flag);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_rdf_brute(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                                 const float* boxes, uint32_t pbc_flags, int B,
                                 const int32_t* ref, int nref, const int32_t* tgt, int ntgt,
                                 float rmin, float rmax, int nbins, uint64_t* counts) {
    hipStream_t s = (hipStream_t)stream;
    if (nbins <= 0 || nbins > VMD_MAX_BINS) return (int)hipErrorInvalidValue;
    if (B <= 0 || nref <= 0 || ntgt <= 0) return 0;
    vmd_brute_params_t p{xyz, frame_stride, row_stride, boxes, pbc_flags, B, ref, nref, tgt, ntgt, {}, counts, g_rdf_raw, nullptr, nullptr};
    p.bin = vmd_make_binning(rmin, rmax, nbins, g_rdf_closed);
    hipLaunchKernelGGL(k_rdf_brute<false>, dim3((nref + 255) / 256, B), dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_rdf_brute_masked(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                                        const float* boxes, uint32_t pbc_flags, int B,
                                        const int32_t* ref, int nref, const uint8_t* ref_mask, const int32_t* tgt, int ntgt,
                                        const uint8_t* tgt_mask, float rmin, float rmax, int nbins, uint64_t* counts) {
    hipStream_t s = (hipStream_t)stream;
    if (nbins <= 0 || nbins > VMD_MAX_BINS) return (int)hipErrorInvalidValue;
    if (B <= 0 || nref <= 0 || ntgt <= 0) return 0;
    if (B > 65535) return (int)hipErrorInvalidValue;
    vmd_brute_params_t p{xyz, frame_stride, row_stride, boxes, pbc_flags, B, ref, nref, tgt, ntgt, {}, counts, g_rdf_raw, ref_mask, tgt_mask};
    p.bin = vmd_make_binning(rmin, rmax, nbins, g_rdf_closed);
    hipLaunchKernelGGL(k_rdf_brute<true>, dim3((nref + 255) / 256, B), dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

static int vmd_within_brute_launch(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                                    const float* boxes, uint32_t pbc_flags, int B,
                                    const int32_t* tgt, int ntgt, const int32_t* ref, int nref,
                                    float rmin, float rmax, int closed, uint32_t* count_out, uint8_t* flags_out, size_t atom_stride = 0) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    if (B > 65535 || !count_out) return (int)hipErrorInvalidValue;
    if (!(rmin >= 0.0f) || !(rmax > rmin)) return (int)hipErrorInvalidValue;
    { const hipError_t e = hipMemsetAsync(count_out, 0, (size_t)B * sizeof(uint32_t), s); if (e != hipSuccess) return (int)e; }
    if (ntgt <= 0 || nref <= 0) return 0;
    vmd_within_brute_params_t p{xyz, frame_stride, row_stride, boxes, pbc_flags, B, tgt, ntgt, ref, nref,
                                vmd_make_within_test(rmin, rmax, closed), count_out, flags_out, atom_stride};
    if (flags_out && atom_stride) hipLaunchKernelGGL((k_within_brute<true, true>), dim3((ntgt + 255) / 256, B), dim3(256), 0, s, p);
    else if (flags_out) hipLaunchKernelGGL(k_within_brute<true>, dim3((ntgt + 255) / 256, B), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_within_brute<false>, dim3((ntgt + 255) / 256, B), dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_within_brute(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                                    const float* boxes, uint32_t pbc_flags, int B,
                                    const int32_t* tgt, int ntgt, const int32_t* ref, int nref,
                                    float rmin, float rmax, int closed, uint32_t* count_out) {
    return vmd_within_brute_launch(stream, xyz, frame_stride, row_stride, boxes, pbc_flags, B, tgt, ntgt, ref, nref, rmin, rmax, closed,
                                   count_out, nullptr);
}

extern "C" int vmd_hip_within_brute_flags(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                                          const float* boxes, uint32_t pbc_flags, int B,
                                          const int32_t* tgt, int ntgt, const int32_t* ref, int nref,
                                          float rmin, float rmax, int closed, uint32_t* count_out, uint8_t* flags_out) {
    if (!flags_out) return (int)hipErrorInvalidValue;
    return vmd_within_brute_launch(stream, xyz, frame_stride, row_stride, boxes, pbc_flags, B, tgt, ntgt, ref, nref, rmin, rmax, closed,
                                   count_out, flags_out);
}

extern "C" int vmd_hip_within_brute_atoms(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                                          const float* boxes, uint32_t pbc_flags, int B,
                                          const int32_t* tgt, int ntgt, const int32_t* ref, int nref,
                                          float rmin, float rmax, int closed, uint32_t* count_out, uint8_t* mask_out, size_t mask_stride) {
    if (!mask_out || !mask_stride) return (int)hipErrorInvalidValue;
    return vmd_within_brute_launch(stream, xyz, frame_stride, row_stride, boxes, pbc_flags, B, tgt, ntgt, ref, nref, rmin, rmax, closed,
                                   count_out, mask_out, mask_stride);
}

// The walk's part of a launch: the cell-sorted copy of R, the test, the padded window of vmd_hip_rdf_pencil and this thread's pencil reach.
// false: the grid or the range is none
static bool vmd_within_walk_fill(vmd_within_walk_params_t& k, const vmd_grid_t& grid, const float* sorted_ref, const uint32_t* cell_start_ref,
                                 int nref_pad, float rmin, float rmax, int closed) {
    if (grid.ny <= 0 || grid.nz <= 0 || grid.nxf <= 0 || !(rmin >= 0.0f) || !(rmax > rmin)) return false;
    k.sref = sorted_ref; k.cs_ref = cell_start_ref; k.nref_pad = nref_pad;
    k.w = vmd_make_within_test(rmin, rmax, closed);
    k.rpad = rmax * 1.0001f + 1.0e-4f;
    k.ry = g_pen_ry; k.rz = g_pen_rz;
    return true;
}
// ... of a kernel that also asks the copy's identity (k_sorted_atoms' table): every argument of the walk side checked, then the fill
static bool vmd_ident_walk_fill(vmd_within_walk_params_t& k, const vmd_grid_t& grid, const float* sorted, const uint32_t* cell_start,
                                const uint32_t* ident, int n, int n_pad, float r, int closed) {
    return sorted && cell_start && ident && n_pad >= n && grid.ncell == grid.nxf * grid.ny * grid.nz &&
           vmd_within_walk_fill(k, grid, sorted, cell_start, n_pad, 0.0f, r, closed);
}
// The lane side of a walk in list order: the list as a cell build on `grid` would read it - raw frame, the GRID's boxes, pbc, index list
// (pat.m = 0; no outputs).
static vmd_cells_params_t vmd_walk_lanes(const float* xyz, size_t frame_stride, size_t row_stride, const float* grid_boxes, uint32_t pbc_flags,
                                         const int32_t* list, int n, const vmd_grid_t& grid) {
    vmd_cells_params_t c{};
    c.xyz = xyz; c.frame_stride = frame_stride; c.row_stride = row_stride; c.boxes = grid_boxes; c.pbc = pbc_flags;
    c.sel = list; c.nsel = n; c.nsel_pad = n; c.grid = grid;
    return c;
}

extern "C" int vmd_hip_within_atoms(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                                    const float* boxes, uint32_t pbc_flags, int B, const int32_t* tgt, int ntgt,
                                    const float* sorted_ref, const uint32_t* cell_start_ref, int nref, int nref_pad, vmd_grid_t grid,
                                    float rmin, float rmax, int closed, uint32_t* count_out, uint8_t* mask_out, size_t mask_stride,
                                    const uint32_t* skip_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    vmd_within_atoms_params_t p{};
    if (B > 65535 || !count_out || !mask_out || !mask_stride || grid.ncell != grid.nxf * grid.ny * grid.nz ||
        !vmd_within_walk_fill(p.k, grid, sorted_ref, cell_start_ref, nref_pad, rmin, rmax, closed)) return (int)hipErrorInvalidValue;
    { const hipError_t e = hipMemsetAsync(count_out, 0, (size_t)B * sizeof(uint32_t), s); if (e != hipSuccess) return (int)e; }
    if (ntgt <= 0) return 0;
    if (nref <= 0 || !sorted_ref || !cell_start_ref) return (int)hipErrorInvalidValue;
    p.c = vmd_walk_lanes(xyz, frame_stride, row_stride, boxes, pbc_flags, tgt, ntgt, grid);
    p.mask = mask_out; p.mask_stride = mask_stride; p.count = count_out; p.skip = skip_flag;
    hipLaunchKernelGGL(k_within_atoms, dim3((ntgt + 255) / 256, B), dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

static int vmd_within_pencil_launch(void* stream, const float* sorted_ref, const uint32_t* cell_start_ref, int nref, int nref_pad,
                                     const float* sorted_tgt, const uint32_t* cell_start_tgt, int ntgt, int ntgt_pad,
                                     const float* boxes, int B, vmd_grid_t grid, float rmin, float rmax, int closed,
                                     uint32_t pbc_flags, uint32_t* count_out, const uint32_t* skip_flag,
                                     uint8_t* flags_out, uint32_t* pen_hits_out) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    vmd_within_pencil_params_t p;
    if (B > 65535 || !count_out || !vmd_within_walk_fill(p.k, grid, sorted_ref, cell_start_ref, nref_pad, rmin, rmax, closed))
        return (int)hipErrorInvalidValue;
    { const hipError_t e = hipMemsetAsync(count_out, 0, (size_t)B * sizeof(uint32_t), s); if (e != hipSuccess) return (int)e; }
    if ((ntgt <= 0 || nref <= 0) && !flags_out) return 0;
    p.stgt = sorted_tgt; p.cs_tgt = cell_start_tgt; p.ntgt_pad = ntgt_pad;
    p.boxes = boxes; p.B = B; p.grid = grid; p.pbc = pbc_flags;
    p.count = count_out; p.skip = skip_flag;
    p.flags = flags_out; p.pen_hits = pen_hits_out;
    if (flags_out) hipLaunchKernelGGL(k_within_pencil<true>, dim3(grid.ny * grid.nz, B), dim3(VMD_WAVE), 0, s, p);
    else hipLaunchKernelGGL(k_within_pencil<false>, dim3(grid.ny * grid.nz, B), dim3(VMD_WAVE), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_within_pencil(void* stream, const float* sorted_ref, const uint32_t* cell_start_ref, int nref, int nref_pad,
                                     const float* sorted_tgt, const uint32_t* cell_start_tgt, int ntgt, int ntgt_pad,
                                     const float* boxes, int B, vmd_grid_t grid, float rmin, float rmax, int closed,
                                     uint32_t pbc_flags, uint32_t* count_out, const uint32_t* skip_flag) {
    return vmd_within_pencil_launch(stream, sorted_ref, cell_start_ref, nref, nref_pad, sorted_tgt, cell_start_tgt, ntgt, ntgt_pad, boxes, B,
                                    grid, rmin, rmax, closed, pbc_flags, count_out, skip_flag, nullptr, nullptr);
}

extern "C" int vmd_hip_within_pencil_flags(void* stream, const float* sorted_ref, const uint32_t* cell_start_ref, int nref, int nref_pad,
                                           const float* sorted_tgt, const uint32_t* cell_start_tgt, int ntgt, int ntgt_pad,
                                           const float* boxes, int B, vmd_grid_t grid, float rmin, float rmax, int closed,
                                           uint32_t pbc_flags, uint32_t* count_out, const uint32_t* skip_flag,
                                           uint8_t* flags_out, uint32_t* pen_hits_out) {
    if (!flags_out || !pen_hits_out || ntgt <= 0 || nref <= 0) return (int)hipErrorInvalidValue;
    return vmd_within_pencil_launch(stream, sorted_ref, cell_start_ref, nref, nref_pad, sorted_tgt, cell_start_tgt, ntgt, ntgt_pad, boxes, B,
                                    grid, rmin, rmax, closed, pbc_flags, count_out, skip_flag, flags_out, pen_hits_out);
}

extern "C" int vmd_hip_shell_compact(void* stream, const uint8_t* flags, const uint32_t* pen_hits, uint32_t* pen_base,
                                     const float* sorted, const uint32_t* cell_start, int nsel_pad, int B, vmd_grid_t grid,
                                     float* sorted_hit, uint32_t* cell_start_hit, const uint32_t* skip_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    if (B > 65535 || !flags || !pen_hits || !pen_base || !sorted || !cell_start || !sorted_hit || !cell_start_hit || nsel_pad <= 0 ||
        grid.ny <= 0 || grid.nz <= 0 || grid.nxf <= 0 || grid.ncell != grid.nxf * grid.ny * grid.nz) return (int)hipErrorInvalidValue;
    const int npen = grid.ny * grid.nz;
    // exclusive prefix of the pencils' hit counts, one block per frame: the cell build's own scan over a table of npen entries
    hipLaunchKernelGGL(k_cells_scan, dim3(B), dim3(1024), 0, s, pen_hits, pen_base, npen);
    VMD_LAUNCH_CHECK();
    vmd_shell_compact_params_t p{flags, pen_base, sorted, cell_start, nsel_pad, sorted_hit, cell_start_hit, B, grid, skip_flag};
    hipLaunchKernelGGL(k_shell_compact, dim3(npen, B), dim3(VMD_WAVE), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_within_to_float(void* stream, const uint32_t* counts, int B, float* out, const uint32_t* skip_flag) {
    if (B <= 0) return 0;
    hipLaunchKernelGGL(k_within_to_float, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, counts, B, out, skip_flag);
    VMD_LAUNCH_CHECK();
    return 0;
}

// ---- K12: hydrogen bonds
extern "C" int vmd_hip_sorted_atoms(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes,
                                    uint32_t pbc_flags, int B, const int32_t* sel, int nsel, const float* sorted, const uint32_t* cell_start,
                                    int nsel_pad, vmd_grid_t grid, uint32_t* ident_out, const uint32_t* skip_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0 || nsel <= 0) return 0;
    if (B > 65535 || !sel || !sorted || !cell_start || !ident_out || nsel_pad < nsel || grid.nxf <= 0 || grid.ny <= 0 || grid.nz <= 0 ||
        grid.ncell != grid.nxf * grid.ny * grid.nz) return (int)hipErrorInvalidValue;
    { const hipError_t e = hipMemsetAsync(ident_out, 0xff, (size_t)B * nsel_pad * sizeof(uint32_t), s); if (e != hipSuccess) return (int)e; }
    vmd_sorted_atoms_params_t p{};
    p.c = vmd_walk_lanes(xyz, frame_stride, row_stride, boxes, pbc_flags, sel, nsel, grid);
    p.c.nsel_pad = nsel_pad;             // (the copy's rows and the table's are the build's)
    p.cell_start = cell_start; p.sorted = sorted; p.ident = ident_out; p.skip = skip_flag;
    hipLaunchKernelGGL(k_sorted_atoms, dim3((nsel + 255) / 256, B), dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

static bool vmd_hbond_args_ok(int B, const int32_t* don, const int32_t* hyd, int npairs, const int32_t* accl, int nacc, float r_da, float c2,
                              const uint32_t* count_out, const uint64_t* acc) {
    return B <= 65535 && don && hyd && npairs > 0 && accl && nacc > 0 && r_da > 0.0f && c2 >= 0.0f && c2 <= 1.0f && count_out && acc;
}

extern "C" int vmd_hip_hbond_atoms(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* grid_boxes,
                                   const float* frame_boxes, uint32_t pbc_flags, int B, const int32_t* don, const int32_t* hyd, int npairs,
                                   const int32_t* accl, int nacc, const float* sorted_acc, const uint32_t* cell_start_acc, int nacc_pad,
                                   const uint32_t* ident, vmd_grid_t grid, float r_da, float c2, int closed, uint32_t* count_out,
                                   uint64_t* acc, const uint32_t* skip_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    vmd_hbond_atoms_params_t p{};
    if (!vmd_hbond_args_ok(B, don, hyd, npairs, accl, nacc, r_da, c2, count_out, acc) || !grid_boxes || !frame_boxes ||
        !vmd_ident_walk_fill(p.k, grid, sorted_acc, cell_start_acc, ident, nacc, nacc_pad, r_da, closed)) return (int)hipErrorInvalidValue;
    { const hipError_t e = hipMemsetAsync(count_out, 0, (size_t)B * sizeof(uint32_t), s); if (e != hipSuccess) return (int)e; }
    p.c = vmd_walk_lanes(xyz, frame_stride, row_stride, grid_boxes, pbc_flags, don, npairs, grid);
    p.fboxes = frame_boxes; p.hyd = hyd; p.accl = accl; p.nacc = nacc; p.ident = ident; p.c2 = c2;
    p.count = count_out; p.acc = acc; p.skip = skip_flag;
    hipLaunchKernelGGL(k_hbond_atoms, dim3((npairs + 255) / 256, B), dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

// the coincidence table in front of an all-pairs launch over `list`
static int vmd_canon_launch(hipStream_t s, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags,
                            int B, const int32_t* list, int n, uint32_t* canon, const uint32_t* skip_flag) {
    vmd_canon_params_t p{xyz, frame_stride, row_stride, boxes, pbc_flags, list, n, canon, skip_flag};
    hipLaunchKernelGGL(k_canon_entries, dim3((n + 255) / 256, B), dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

static int vmd_hbond_brute_launch(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes,
                                  uint32_t pbc_flags, int B, const int32_t* don, const int32_t* hyd, int npairs, const int32_t* accl, int nacc,
                                  uint32_t* canon, float r_da, float c2, int closed, uint32_t* count_out, uint64_t* acc,
                                  const uint32_t* skip_flag, uint32_t* list, uint32_t list_cap, uint32_t* list_count) {
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = vmd_canon_launch(s, xyz, frame_stride, row_stride, boxes, pbc_flags, B, accl, nacc, canon, skip_flag)) return rc;
    vmd_hbond_brute_params_t p{xyz, frame_stride, row_stride, boxes, pbc_flags, don, hyd, npairs, accl, nacc, canon,
                               vmd_make_within_test(0.0f, r_da, closed), c2, count_out, acc, skip_flag, list, list_cap, list_count};
    if (list) hipLaunchKernelGGL(k_hbond_brute<true>, dim3((npairs + 255) / 256, B), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_hbond_brute<false>, dim3((npairs + 255) / 256, B), dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_hbond_brute(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes,
                                   uint32_t pbc_flags, int B, const int32_t* don, const int32_t* hyd, int npairs, const int32_t* accl, int nacc,
                                   uint32_t* canon, float r_da, float c2, int closed, uint32_t* count_out, uint64_t* acc,
                                   const uint32_t* skip_flag) {
    if (B <= 0) return 0;
    if (!vmd_hbond_args_ok(B, don, hyd, npairs, accl, nacc, r_da, c2, count_out, acc) || !canon || !boxes) return (int)hipErrorInvalidValue;
    { const hipError_t e = hipMemsetAsync(count_out, 0, (size_t)B * sizeof(uint32_t), (hipStream_t)stream); if (e != hipSuccess) return (int)e; }
    return vmd_hbond_brute_launch(stream, xyz, frame_stride, row_stride, boxes, pbc_flags, B, don, hyd, npairs, accl, nacc, canon, r_da, c2,
                                  closed, count_out, acc, skip_flag, nullptr, 0, nullptr);
}

extern "C" int vmd_hip_hbond_list(void* stream, const float* xyz, size_t row_stride, const float* box, uint32_t pbc_flags, const int32_t* don,
                                  const int32_t* hyd, int npairs, const int32_t* accl, int nacc, uint32_t* canon, float r_da, float c2,
                                  int closed, uint32_t* list, uint32_t list_cap, uint32_t* list_count) {
    if (!don || !hyd || npairs <= 0 || !accl || nacc <= 0 || !(r_da > 0.0f) || !canon || !box || !list || !list_count)
        return (int)hipErrorInvalidValue;
    { const hipError_t e = hipMemsetAsync(list_count, 0, sizeof(uint32_t), (hipStream_t)stream); if (e != hipSuccess) return (int)e; }
    return vmd_hbond_brute_launch(stream, xyz, 0, row_stride, box, pbc_flags, 1, don, hyd, npairs, accl, nacc, canon, r_da, c2, closed, nullptr,
                                  nullptr, nullptr, list, list_cap, list_count);
}

extern "C" int vmd_hip_hbond_finish(void* stream, const uint32_t* counts, int B, float* out, uint64_t* frames_row, const uint32_t* skip_flag) {
    if (B <= 0) return 0;
    if (!counts || !out || !frames_row) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hbond_finish, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, counts, B, out, frames_row, skip_flag);
    VMD_LAUNCH_CHECK();
    return 0;
}

// ---- K13: solvent-accessible surface area
static bool vmd_sasa_args_ok(int B, const int32_t* meas, int nmeas, const int32_t* envl, int nenv, const float* r_meas, const float* r_env,
                             float rmax_env, const float* points, int npoints, float r_cut) {
    return B <= 65535 && meas && nmeas > 0 && envl && nenv > 0 && r_meas && r_env && rmax_env > 0.0f && points && npoints >= 1 &&
           npoints <= VMD_SASA_POINTS_MAX && r_cut > 0.0f;
}

extern "C" int vmd_hip_sasa_atoms(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* grid_boxes,
                                  uint32_t pbc_flags, int B, const int32_t* meas, int nmeas, const int32_t* envl, int nenv,
                                  const float* sorted_env, const uint32_t* cell_start_env, int nenv_pad, const uint32_t* ident,
                                  vmd_grid_t grid, const float* r_meas, const float* r_env, float rmax_env, const uint32_t* weight,
                                  const float* points, int npoints, float r_cut, int closed, uint64_t* total_out, uint64_t* acc,
                                  const uint32_t* skip_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    vmd_sasa_atoms_params_t p{};
    if (!vmd_sasa_args_ok(B, meas, nmeas, envl, nenv, r_meas, r_env, rmax_env, points, npoints, r_cut) || !weight || !total_out || !acc ||
        !grid_boxes || !vmd_ident_walk_fill(p.k, grid, sorted_env, cell_start_env, ident, nenv, nenv_pad, r_cut, closed))
        return (int)hipErrorInvalidValue;
    { const hipError_t e = hipMemsetAsync(total_out, 0, (size_t)B * sizeof(uint64_t), s); if (e != hipSuccess) return (int)e; }
    p.c = vmd_walk_lanes(xyz, frame_stride, row_stride, grid_boxes, pbc_flags, meas, nmeas, grid);
    p.envl = envl; p.nenv = nenv; p.ident = ident; p.r_meas = r_meas; p.r_env = r_env; p.rmax_env = rmax_env; p.weight = weight;
    p.points = points; p.npoints = npoints; p.total = total_out; p.acc = acc; p.skip = skip_flag;
    const dim3 g((nmeas + 255) / 256, B);
    if (npoints <= 128) hipLaunchKernelGGL(k_sasa_atoms<4>, g, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_sasa_atoms<VMD_SASA_POINTS_MAX / 32>, g, dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

static int vmd_sasa_brute_launch(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes,
                                 uint32_t pbc_flags, int B, const int32_t* meas, int nmeas, const int32_t* envl, int nenv, uint32_t* canon,
                                 const float* r_meas, const float* r_env, float rmax_env, const uint32_t* weight, const float* points,
                                 int npoints, float r_cut, int closed, uint64_t* total_out, uint64_t* acc, const uint32_t* skip_flag,
                                 uint32_t* counts) {
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = vmd_canon_launch(s, xyz, frame_stride, row_stride, boxes, pbc_flags, B, envl, nenv, canon, skip_flag)) return rc;
    vmd_sasa_brute_params_t p{xyz, frame_stride, row_stride, boxes, pbc_flags, meas, nmeas, envl, nenv, canon, r_meas, r_env, rmax_env,
                              weight, points, npoints, vmd_make_within_test(0.0f, r_cut, closed), total_out, acc, skip_flag, counts};
    if (counts) hipLaunchKernelGGL(k_sasa_brute<true>, dim3((nmeas + 255) / 256, B), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_sasa_brute<false>, dim3((nmeas + 255) / 256, B), dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_sasa_brute(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes,
                                  uint32_t pbc_flags, int B, const int32_t* meas, int nmeas, const int32_t* envl, int nenv, uint32_t* canon,
                                  const float* r_meas, const float* r_env, float rmax_env, const uint32_t* weight, const float* points,
                                  int npoints, float r_cut, int closed, uint64_t* total_out, uint64_t* acc, const uint32_t* skip_flag) {
    if (B <= 0) return 0;
    if (!vmd_sasa_args_ok(B, meas, nmeas, envl, nenv, r_meas, r_env, rmax_env, points, npoints, r_cut) || !weight || !total_out || !acc ||
        !canon || !boxes) return (int)hipErrorInvalidValue;
    { const hipError_t e = hipMemsetAsync(total_out, 0, (size_t)B * sizeof(uint64_t), (hipStream_t)stream); if (e != hipSuccess) return (int)e; }
    return vmd_sasa_brute_launch(stream, xyz, frame_stride, row_stride, boxes, pbc_flags, B, meas, nmeas, envl, nenv, canon, r_meas, r_env,
                                 rmax_env, weight, points, npoints, r_cut, closed, total_out, acc, skip_flag, nullptr);
}

extern "C" int vmd_hip_sasa_list(void* stream, const float* xyz, size_t row_stride, const float* box, uint32_t pbc_flags, const int32_t* meas,
                                 int nmeas, const int32_t* envl, int nenv, uint32_t* canon, const float* r_meas, const float* r_env,
                                 float rmax_env, const float* points, int npoints, float r_cut, int closed, uint32_t* counts_out) {
    // (the LIST instantiation reads no weight and writes no total)
    if (!vmd_sasa_args_ok(1, meas, nmeas, envl, nenv, r_meas, r_env, rmax_env, points, npoints, r_cut) || !canon || !box ||
        !counts_out) return (int)hipErrorInvalidValue;
    return vmd_sasa_brute_launch(stream, xyz, 0, row_stride, box, pbc_flags, 1, meas, nmeas, envl, nenv, canon, r_meas, r_env, rmax_env,
                                 nullptr, points, npoints, r_cut, closed, nullptr, nullptr, nullptr, counts_out);
}

extern "C" int vmd_hip_sasa_finish(void* stream, const uint64_t* totals, int B, float* out, uint64_t* frames_row, const uint32_t* skip_flag) {
    if (B <= 0) return 0;
    if (!totals || !out || !frames_row) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sasa_finish, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, totals, B, out, frames_row, skip_flag);
    VMD_LAUNCH_CHECK();
    return 0;
}

// ---- K14: residue contact maps
static bool vmd_contact_args_ok(int B, const int32_t* ent, const int32_t* grp, int nent, int ngroups, uint32_t min_sep, float r_cut,
                                const uint32_t* bits) {
    return B <= 65535 && ent && grp && nent > 0 && ngroups >= 2 && ngroups <= 2048 && min_sep >= 1 && min_sep < (uint32_t)ngroups &&
           r_cut > 0.0f && bits;
}
static uint32_t vmd_contact_pairs(int ngroups) { return (uint32_t)ngroups * (uint32_t)(ngroups - 1) / 2u; }

extern "C" int vmd_hip_contact_atoms(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* grid_boxes,
                                     uint32_t pbc_flags, int B, const int32_t* ent, const int32_t* grp, int nent, int ngroups,
                                     uint32_t min_sep, const float* sorted, const uint32_t* cell_start, int nent_pad, const uint32_t* ident,
                                     vmd_grid_t grid, float r_cut, int closed, int lds_rows, uint32_t* bits, const uint32_t* skip_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    vmd_contact_atoms_params_t p{};
    if (!vmd_contact_args_ok(B, ent, grp, nent, ngroups, min_sep, r_cut, bits) || !grid_boxes ||
        !vmd_ident_walk_fill(p.k, grid, sorted, cell_start, ident, nent, nent_pad, r_cut, closed)) return (int)hipErrorInvalidValue;
    const uint32_t W = (vmd_contact_pairs(ngroups) + 31u) / 32u;
    { const hipError_t e = hipMemsetAsync(bits, 0, (size_t)B * W * sizeof(uint32_t), s); if (e != hipSuccess) return (int)e; }
    p.c = vmd_walk_lanes(xyz, frame_stride, row_stride, grid_boxes, pbc_flags, ent, nent, grid);
    p.grp = grp; p.ngroups = (uint32_t)ngroups; p.min_sep = min_sep; p.ident = ident; p.bits = bits; p.W = W; p.skip = skip_flag;
    if (lds_rows) hipLaunchKernelGGL(k_contact_atoms<true>, dim3((nent + 255) / 256, B), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_contact_atoms<false>, dim3((nent + 255) / 256, B), dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_contact_brute(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes,
                                     uint32_t pbc_flags, int B, const int32_t* ent, const int32_t* grp, int nent, int ngroups,
                                     uint32_t min_sep, uint32_t* canon, float r_cut, int closed, uint32_t* bits, const uint32_t* skip_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    if (!vmd_contact_args_ok(B, ent, grp, nent, ngroups, min_sep, r_cut, bits) || !canon || !boxes) return (int)hipErrorInvalidValue;
    const uint32_t W = (vmd_contact_pairs(ngroups) + 31u) / 32u;
    { const hipError_t e = hipMemsetAsync(bits, 0, (size_t)B * W * sizeof(uint32_t), s); if (e != hipSuccess) return (int)e; }
    if (const int rc = vmd_canon_launch(s, xyz, frame_stride, row_stride, boxes, pbc_flags, B, ent, nent, canon, skip_flag)) return rc;
    vmd_contact_brute_params_t p{xyz, frame_stride, row_stride, boxes, pbc_flags, ent, grp, nent, (uint32_t)ngroups, min_sep, canon,
                                 vmd_make_within_test(0.0f, r_cut, closed), bits, W, skip_flag};
    hipLaunchKernelGGL(k_contact_brute, dim3((nent + 255) / 256, B), dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_contact_finish(void* stream, const uint32_t* bits, int B, int ngroups, const uint32_t* native, int nnative,
                                      uint32_t* counts, float* out_count, float* out_q, uint64_t* acc, const uint32_t* skip_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    if (B > 65535 || !bits || ngroups < 2 || ngroups > 2048 || nnative < 0 || (nnative > 0 && (!native || !out_q)) || !counts || !out_count ||
        !acc) return (int)hipErrorInvalidValue;
    const uint32_t P = vmd_contact_pairs(ngroups), W = (P + 31u) / 32u;
    { const hipError_t e = hipMemsetAsync(counts, 0, 2 * (size_t)B * sizeof(uint32_t), s); if (e != hipSuccess) return (int)e; }
    vmd_contact_finish_params_t q{bits, W, P, B, native, nnative, counts, out_count, nnative > 0 ? out_q : nullptr, acc, skip_flag};
    hipLaunchKernelGGL(k_contact_finish_rows, dim3((W + 255u) / 256u), dim3(256), 0, s, q);
    VMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_contact_finish_frames, dim3((W + 255u) / 256u + ((uint32_t)nnative + 255u) / 256u, B), dim3(256), 0, s, q);
    VMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_contact_finish_out, dim3((B + 255) / 256), dim3(256), 0, s, q);
    VMD_LAUNCH_CHECK();
    return 0;
}

// ---- K15: clusters of groups
static bool vmd_cluster_args_ok(int B, const int32_t* ent, const int32_t* grp, int nent, int ngroups, float r_cut, const uint32_t* parent) {
    return B <= 65535 && ent && grp && nent > 0 && ngroups >= 1 && ngroups <= (1 << 24) && r_cut > 0.0f && parent;
}
// parent[b][g] = g, in front of every launch that unites
static int vmd_cluster_init(hipStream_t s, int B, int ngroups, uint32_t* parent, const uint32_t* skip_flag) {
    hipLaunchKernelGGL(k_cluster_init, dim3((ngroups + 255) / 256, B), dim3(256), 0, s, parent, (uint32_t)ngroups, skip_flag);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_cluster_atoms(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* grid_boxes,
                                     uint32_t pbc_flags, int B, const int32_t* ent, const int32_t* grp, int nent, int ngroups,
                                     const float* sorted, const uint32_t* cell_start, int nent_pad, const uint32_t* ident, vmd_grid_t grid,
                                     float r_cut, int closed, int skip_same, uint32_t* parent, const uint32_t* skip_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    vmd_cluster_atoms_params_t p{};
    if (!vmd_cluster_args_ok(B, ent, grp, nent, ngroups, r_cut, parent) || !grid_boxes ||
        !vmd_ident_walk_fill(p.k, grid, sorted, cell_start, ident, nent, nent_pad, r_cut, closed)) return (int)hipErrorInvalidValue;
    if (const int rc = vmd_cluster_init(s, B, ngroups, parent, skip_flag)) return rc;
    p.c = vmd_walk_lanes(xyz, frame_stride, row_stride, grid_boxes, pbc_flags, ent, nent, grid);
    p.grp = grp; p.ngroups = (uint32_t)ngroups; p.ident = ident; p.parent = parent; p.skip = skip_flag;
    if (skip_same) hipLaunchKernelGGL(k_cluster_atoms<true>, dim3((nent + 255) / 256, B), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_cluster_atoms<false>, dim3((nent + 255) / 256, B), dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_cluster_brute(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes,
                                     uint32_t pbc_flags, int B, const int32_t* ent, const int32_t* grp, int nent, int ngroups, float r_cut,
                                     int closed, uint32_t* parent, const uint32_t* skip_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    if (!vmd_cluster_args_ok(B, ent, grp, nent, ngroups, r_cut, parent) || !boxes) return (int)hipErrorInvalidValue;
    if (const int rc = vmd_cluster_init(s, B, ngroups, parent, skip_flag)) return rc;
    vmd_cluster_brute_params_t p{xyz, frame_stride, row_stride, boxes, pbc_flags, ent, grp, nent, (uint32_t)ngroups,
                                 vmd_make_within_test(0.0f, r_cut, closed), parent, skip_flag};
    hipLaunchKernelGGL(k_cluster_brute, dim3((nent + 255) / 256, B), dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_cluster_finish(void* stream, const uint32_t* parent, uint32_t* root, uint32_t* size, int B, int ngroups,
                                      uint32_t* counts, float* out_count, float* out_largest, uint64_t* acc, int wave_singles,
                                      const uint32_t* skip_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    if (B > 65535 || !parent || !root || !size || ngroups < 1 || ngroups > (1 << 24) || !counts) return (int)hipErrorInvalidValue;
    { const hipError_t e = hipMemsetAsync(size, 0, (size_t)B * (size_t)ngroups * sizeof(uint32_t), s); if (e != hipSuccess) return (int)e; }
    { const hipError_t e = hipMemsetAsync(counts, 0, 2 * (size_t)B * sizeof(uint32_t), s); if (e != hipSuccess) return (int)e; }
    vmd_cluster_finish_params_t q{parent, root, size, (uint32_t)ngroups, B, counts, out_count, out_largest, acc, skip_flag};
    const dim3 grid((ngroups + 255) / 256, B);
    hipLaunchKernelGGL(k_cluster_finish_roots, grid, dim3(256), 0, s, q);
    VMD_LAUNCH_CHECK();
    if (wave_singles) hipLaunchKernelGGL(k_cluster_finish_count<true>, grid, dim3(256), 0, s, q);
    else hipLaunchKernelGGL(k_cluster_finish_count<false>, grid, dim3(256), 0, s, q);
    VMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cluster_finish_out, dim3((B + 255) / 256), dim3(256), 0, s, q);
    VMD_LAUNCH_CHECK();
    return 0;
}

// ---- K16: the position table's rows of a batch, and the two launches of a query
extern "C" int vmd_hip_msd_gather(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes,
                                  uint32_t pbc_flags, int B, const int32_t* idx, int n, float* rows) {
    if (B <= 0) return 0;
    if (B > 65535 || !xyz || !boxes || !idx || !rows || n < 1 || n > VMD_MSD_MAX_ATOMS) return (int)hipErrorInvalidValue;
    vmd_msd_gather_params_t p{vmd_frames(xyz, frame_stride, row_stride, boxes, pbc_flags, B), idx, n, rows};
    hipLaunchKernelGGL(k_msd_gather, dim3((unsigned)((3 * n + VMD_BOX_STRIDE + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_msd_unwrap(void* stream, const float* rows, int F, int n, int32_t* counts) {
    if (F <= 0) return 0;
    if (!rows || !counts || n < 1 || n > VMD_MSD_MAX_ATOMS) return (int)hipErrorInvalidValue;
    vmd_msd_unwrap_params_t p{rows, F, n, counts};
    hipLaunchKernelGGL(k_msd_unwrap, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_msd_tile(int* atoms, int* origins, int* lags) {
    if (atoms) *atoms = VMD_MSD_A;
    if (origins) *origins = VMD_MSD_SO;
    if (lags) *lags = VMD_MSD_LC;
    return 0;
}

extern "C" int vmd_hip_msd_lags(void* stream, const float* rows, const int32_t* counts, int F, int n, int max_lag, int origin_stride,
                                uint64_t* sums) {
    if (F <= 0) return 0;
    const long long spans = ((long long)F + VMD_MSD_SO - 1) / VMD_MSD_SO, chunks = (long long)max_lag / VMD_MSD_LC + 1;
    if (!rows || !counts || !sums || n < 1 || n > VMD_MSD_MAX_ATOMS || max_lag < 0 || max_lag >= F || origin_stride < 1 || spans > 65535 ||
        chunks > 65535) return (int)hipErrorInvalidValue;
    // enough blocks to fill the device several times over, few enough that the atomics of a lag row stay a small part of its terms
    const long long tiles = ((long long)n + VMD_MSD_A - 1) / VMD_MSD_A;
    const long long gx = std::min(tiles, std::max(1LL, 8192LL / (spans * chunks)));
    vmd_msd_lags_params_t p{rows, counts, F, n, max_lag, origin_stride, (unsigned long long*)sums};
    hipLaunchKernelGGL(k_msd_lags, dim3((unsigned)gx, (unsigned)spans, (unsigned)chunks), dim3(VMD_MSD_LC), 0, (hipStream_t)stream, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

// ---- K9: one term pass of a shell expression, and the finish
static bool vmd_expr_term_ok(int B, int term, uint32_t live, const uint8_t* bits, size_t stride, float rmin, float rmax) {
    return B <= 65535 && term >= 0 && term < 4 && live <= 0xffffu && bits && stride && rmin >= 0.0f && rmax > rmin;
}

extern "C" int vmd_hip_within_atoms_expr(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                                         const float* boxes, uint32_t pbc_flags, int B, const int32_t* tgt, int ntgt,
                                         const float* sorted_ref, const uint32_t* cell_start_ref, int nref, int nref_pad, vmd_grid_t grid,
                                         float rmin, float rmax, int closed, int term, uint32_t live, uint8_t* bits, size_t stride,
                                         const uint32_t* skip_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0 || ntgt <= 0 || !live) return 0;
    vmd_within_atoms_expr_params_t p{};
    if (!vmd_expr_term_ok(B, term, live, bits, stride, rmin, rmax) || grid.ncell != grid.nxf * grid.ny * grid.nz || nref <= 0 ||
        !sorted_ref || !cell_start_ref || !vmd_within_walk_fill(p.k, grid, sorted_ref, cell_start_ref, nref_pad, rmin, rmax, closed))
        return (int)hipErrorInvalidValue;
    p.c = vmd_walk_lanes(xyz, frame_stride, row_stride, boxes, pbc_flags, tgt, ntgt, grid);
    p.bits = bits; p.stride = stride; p.term = term; p.live = live; p.skip = skip_flag;
    hipLaunchKernelGGL(k_within_atoms_expr, dim3((ntgt + 255) / 256, B), dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_within_brute_expr(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                                         const float* boxes, uint32_t pbc_flags, int B,
                                         const int32_t* tgt, int ntgt, const int32_t* ref, int nref,
                                         float rmin, float rmax, int closed, int term, uint32_t live, uint8_t* bits, size_t stride,
                                         const uint32_t* skip_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0 || ntgt <= 0 || nref <= 0 || !live) return 0;
    if (!vmd_expr_term_ok(B, term, live, bits, stride, rmin, rmax)) return (int)hipErrorInvalidValue;
    vmd_within_brute_expr_params_t p{xyz, frame_stride, row_stride, boxes, pbc_flags, B, tgt, ntgt, ref, nref,
                                     vmd_make_within_test(rmin, rmax, closed), bits, stride, term, live, skip_flag};
    hipLaunchKernelGGL(k_within_brute_expr, dim3((ntgt + 63) / 64, B), dim3(VMD_WAVE), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_shell_expr_finish(void* stream, int B, const int32_t* tgt, int ntgt, const uint8_t* bits, uint32_t truth,
                                         uint8_t* mask_out, size_t stride, uint32_t* count_out, const uint32_t* skip_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0) return 0;
    if (B > 65535 || !count_out || !bits || !mask_out || !stride || truth > 0xffffu) return (int)hipErrorInvalidValue;
    { const hipError_t e = hipMemsetAsync(count_out, 0, (size_t)B * sizeof(uint32_t), s); if (e != hipSuccess) return (int)e; }
    if (ntgt <= 0) return 0;
    vmd_shell_expr_finish_params_t p{tgt, ntgt, bits, mask_out, stride, truth, count_out, skip_flag};
    hipLaunchKernelGGL(k_shell_expr_finish, dim3((ntgt + 255) / 256, B), dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_sdf_align(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                                 const float* boxes, uint32_t pbc_flags, int B,
                                 const int32_t* structs, const float* mass, int K, int m, const double* ref_pose,
                                 float* R32, float* c32, double* M64, float* group,
                                 const int32_t* tree_order, const int32_t* tree_parent, double* tree_pos) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0 || K <= 0 || m <= 0) return 0;
    if ((tree_order != nullptr) != (tree_parent != nullptr) || (tree_order && !tree_pos)) return (int)hipErrorInvalidValue;
    vmd_align_params_t p{vmd_frames(xyz, frame_stride, row_stride, boxes, pbc_flags, B), structs, mass, K, m, ref_pose, R32, c32, M64, tree_order, tree_parent, tree_pos};
    hipLaunchKernelGGL(k_sdf_align, dim3((B * K + 63) / 64), dim3(64), 0, s, p);
    VMD_LAUNCH_CHECK();
    if (group) {
        hipLaunchKernelGGL(k_sdf_group, dim3((B + 63) / 64), dim3(64), 0, s, (const float*)c32, boxes, pbc_flags, B, K, group);
        VMD_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int vmd_hip_sdf_ref_pose(void* stream, const float* xyz, size_t row_stride, const float* box, uint32_t pbc_flags,
                                    const int32_t* struct0, const float* mass0, int m, double* ref_pose,
                                    const int32_t* tree_order, const int32_t* tree_parent) {
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sdf_ref_pose, dim3(1), dim3(64), 0, s, xyz, row_stride, box, pbc_flags, struct0, mass0, m, ref_pose, tree_order, tree_parent);
    VMD_LAUNCH_CHECK();
    return 0;
}

static int g_sdf_nt = 0;        // the scatter's gathers as non-temporal loads (A/B: profiles/r03i_ab_c4.txt)
extern "C" int vmd_hip_set_sdf_nt(int on) { const int old = g_sdf_nt; g_sdf_nt = on ? 1 : 0; return old; }
static int g_sdf_rows = 0;      // row-streaming scatter for arithmetic-progression targets: groups of 4 atoms per thread (0 = off, 1 / 2 / 4)
extern "C" int vmd_hip_set_sdf_rows(int n) { const int old = g_sdf_rows; if (n == 0 || n == 1 || n == 2 || n == 4) g_sdf_rows = n; return old; }
static int g_sdf_wave = 0;      // 1: per-wave instead of per-block compaction of the group test's survivors (no block barrier);
                                // 2: the persistent streaming kernel (k_sdf_scatter_stream) on 2 048 blocks, n >= 16: on n blocks
extern "C" int vmd_hip_set_sdf_wave(int on) { const int old = g_sdf_wave; g_sdf_wave = on < 0 ? 0 : (on > 65535 ? 65535 : on); return old; }
static int g_sdf_ilp = 4;
extern "C" int vmd_hip_set_sdf_ilp(int n) { const int old = g_sdf_ilp; if (n == 4 || n == 8 || n == 16) g_sdf_ilp = n; return old; }

#include <type_traits>
static vmd_scatter_params_t vmd_sdf_params(const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags, int B,
                                           const int32_t* structs, int K, int m, const float* R32, const float* c32,
                                           const int32_t* tgt, const int8_t* owner, int ntgt, float extent, int dim, uint64_t* volume,
                                           const float* group, int tgt_first, int tgt_stride, int unowned) {
    return vmd_scatter_params_t{xyz, frame_stride, row_stride, boxes, pbc_flags, B, structs, K, m, R32, c32, tgt, owner, ntgt, extent, dim,
                                (unsigned long long*)volume, group, tgt_first, tgt_stride, unowned, g_sdf_nt};
}

// (sdf_ilp, arith) -> template arguments: f(std::integral_constant<int, ILP>, std::bool_constant<ARITH>).  The block kernel exists for
// ILP 4 / 8 / 16 (WITH_16), the wave and stream kernels for 8, and anything else means 4
template <bool WITH_16, class F>
static void vmd_sdf_with_ilp_arith(bool arith, F f) {
    auto with_arith = [&](auto ilp) { if (arith) f(ilp, std::true_type{}); else f(ilp, std::false_type{}); };
    if constexpr (WITH_16) { if (g_sdf_ilp == 16) return with_arith(std::integral_constant<int, 16>{}); }
    if (g_sdf_ilp == 8) with_arith(std::integral_constant<int, 8>{});
    else with_arith(std::integral_constant<int, 4>{});
}

template <bool MASKED>
static void vmd_sdf_launch_block(hipStream_t s, const typename vmd_scatter_arg<MASKED>::type& p) {
    vmd_sdf_with_ilp_arith<true>(p.tgt_stride > 0, [&](auto ilp, auto arith) {
        constexpr int ILP = decltype(ilp)::value;
        hipLaunchKernelGGL((k_sdf_scatter<ILP, decltype(arith)::value, MASKED>), dim3((p.ntgt + 256 * ILP - 1) / (256 * ILP), p.B), dim3(256), 0, s, p);
    });
}

extern "C" int vmd_hip_sdf_scatter(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                                   const float* boxes, uint32_t pbc_flags, int B,
                                   const int32_t* structs, int K, int m, const float* R32, const float* c32,
                                   const int32_t* tgt, const int8_t* owner, int ntgt, float extent, int dim, uint64_t* volume,
                                   const float* group, const uint8_t* atom_tag, int tgt_first, int tgt_stride, int unowned) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0 || K <= 0 || ntgt <= 0) return 0;
    const vmd_scatter_params_t p = vmd_sdf_params(xyz, frame_stride, row_stride, boxes, pbc_flags, B, structs, K, m, R32, c32, tgt, owner, ntgt,
                                                  extent, dim, volume, group, tgt_first, tgt_stride, unowned);
    if (atom_tag) {
        const int natoms4 = (int)(row_stride / 4);       // rows are padded to a multiple of 64 floats; the tag array covers the padding
        hipLaunchKernelGGL(k_sdf_scatter_dense, dim3((natoms4 + 255) / 256, B), dim3(256), 0, s, p, atom_tag, natoms4);
        VMD_LAUNCH_CHECK();
        return 0;
    }
    const bool arith = tgt_stride > 0;
    if (arith && g_sdf_rows && tgt_stride <= 4 && ((uintptr_t)xyz & 15u) == 0 && row_stride % 4 == 0 && frame_stride % 4 == 0) {
        // the rows are read in full anyway: stream them with 16-byte loads (stride <= 4: every group of 4 atoms holds a target)
        const int g_first = tgt_first / 4;
        const int g_last = (int)(((long long)tgt_first + (long long)(ntgt - 1) * tgt_stride) / 4);
        const int ngroups = g_last - g_first + 1;
        if (g_sdf_rows == 2) hipLaunchKernelGGL((k_sdf_scatter_rows<2>), dim3((ngroups + 511) / 512, B), dim3(256), 0, s, p, g_first, ngroups);
        else if (g_sdf_rows == 4) hipLaunchKernelGGL((k_sdf_scatter_rows<4>), dim3((ngroups + 1023) / 1024, B), dim3(256), 0, s, p, g_first, ngroups);
        else hipLaunchKernelGGL((k_sdf_scatter_rows<1>), dim3((ngroups + 255) / 256, B), dim3(256), 0, s, p, g_first, ngroups);
        VMD_LAUNCH_CHECK();
        return 0;
    }
    if (g_sdf_wave >= 2) {
        vmd_sdf_with_ilp_arith<false>(arith, [&](auto ilp, auto ar) {
            constexpr int ILP = decltype(ilp)::value;
            const int tiles_per_frame = (ntgt + VMD_WAVE * ILP - 1) / (VMD_WAVE * ILP);
            const long long ntiles = (long long)tiles_per_frame * B;
            long long nblocks = g_sdf_wave >= 16 ? g_sdf_wave : 2048;
            if (nblocks > (ntiles + 3) / 4) nblocks = (ntiles + 3) / 4;
            hipLaunchKernelGGL((k_sdf_scatter_stream<ILP, decltype(ar)::value>), dim3((unsigned)nblocks), dim3(256), 0, s, p, tiles_per_frame);
        });
    } else if (g_sdf_wave) {
        vmd_sdf_with_ilp_arith<false>(arith, [&](auto ilp, auto ar) {
            constexpr int ILP = decltype(ilp)::value;
            hipLaunchKernelGGL((k_sdf_scatter_wave<ILP, decltype(ar)::value>), dim3((ntgt + 256 * ILP - 1) / (256 * ILP), B), dim3(256), 0, s, p);
        });
    } else {
        vmd_sdf_launch_block<false>(s, p);
    }
    VMD_LAUNCH_CHECK();
    return 0;
}

// the masked scatter of a shell target: always k_sdf_scatter<ILP, ARITH, true> - the _wave, _stream, _rows and _dense variants have
// no masked form and are never chosen for a shell, whatever their switches say
extern "C" int vmd_hip_sdf_scatter_masked(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                                          const float* boxes, uint32_t pbc_flags, int B,
                                          const int32_t* structs, int K, int m, const float* R32, const float* c32,
                                          const int32_t* tgt, const int8_t* owner, int ntgt, float extent, int dim, uint64_t* volume,
                                          const float* group, int tgt_first, int tgt_stride, int unowned,
                                          const uint8_t* mask, size_t mask_stride, const uint32_t* skip_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0 || K <= 0 || ntgt <= 0) return 0;
    if (B > 65535 || !mask || !mask_stride) return (int)hipErrorInvalidValue;
    vmd_scatter_masked_params_t p;
    (vmd_scatter_params_t&)p = vmd_sdf_params(xyz, frame_stride, row_stride, boxes, pbc_flags, B, structs, K, m, R32, c32, tgt, owner, ntgt,
                                              extent, dim, volume, group, tgt_first, tgt_stride, unowned);
    p.mask = mask; p.mask_stride = mask_stride; p.skip = skip_flag;
    vmd_sdf_launch_block<true>(s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_distance(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                                const float* boxes, uint32_t pbc_flags, int B, int kind, int P, int per,
                                const int32_t* a, const float* mass_a, const int32_t* aoff,
                                const int32_t* b, const float* mass_b, const int32_t* boff, float* out) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0 || P <= 0 || per <= 0) return 0;
    if ((long long)B * P > 0x7fffffffLL) return (int)hipErrorInvalidValue;     // B * P is an int below, and on grid.x
    vmd_dist_params_t p{vmd_frames(xyz, frame_stride, row_stride, boxes, pbc_flags, B), a, mass_a, aoff, b, mass_b, boff, P, per, out};
    switch (kind) {
    case 0: hipLaunchKernelGGL(k_distance_com, dim3((B * P + 63) / 64), dim3(64), 0, s, p); break;
    case 1: hipLaunchKernelGGL((k_distance_minmax<false>), dim3(B * P), dim3(256), 0, s, p); break;
    case 2: hipLaunchKernelGGL((k_distance_minmax<true>), dim3(B * P), dim3(256), 0, s, p); break;
    case 3:
        if ((per + 255) / 256 > 65535) return (int)hipErrorInvalidValue;      // > 16.7M pairs per context: not a distance_pair population
        hipLaunchKernelGGL(k_distance_pair, dim3((unsigned)(B * P), (unsigned)((per + 255) / 256)), dim3(256), 0, s, p);
        break;
    default: return (int)hipErrorInvalidValue;
    }
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_geometry(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                                const float* boxes, uint32_t pbc_flags, int B, int nargs, int P,
                                const int32_t* const* sets, const float* const* masses, const int32_t* const* offsets, int radians,
                                float* out) {
    if (B <= 0 || P <= 0) return 0;
    if ((nargs != 3 && nargs != 4) || !sets || !masses || !offsets || (long long)B * P > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    vmd_geom_params_t p{};
    p.f = vmd_frames(xyz, frame_stride, row_stride, boxes, pbc_flags, B); p.P = P;
    for (int k = 0; k < nargs; ++k) {
        if (!sets[k] || !masses[k] || !offsets[k]) return (int)hipErrorInvalidValue;
        p.set[k] = sets[k]; p.mass[k] = masses[k]; p.off[k] = offsets[k];
    }
    p.radians = radians; p.out = out;
    const dim3 g((unsigned)(((long long)B * P + 63) / 64));
    if (nargs == 3) hipLaunchKernelGGL((k_geom<3>), g, dim3(64), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((k_geom<4>), g, dim3(64), 0, (hipStream_t)stream, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_backbone_angles(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes,
                                       uint32_t pbc_flags, int B, int nseg, const int32_t* n, const int32_t* ca, const int32_t* c,
                                       const uint8_t* link, float* out) {
    if (B <= 0 || nseg <= 0) return 0;
    if (!xyz || !boxes || !n || !ca || !c || !link || !out || (long long)B * nseg > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    vmd_bb_params_t p{vmd_frames(xyz, frame_stride, row_stride, boxes, pbc_flags, B), n, ca, c, link, nseg, out};
    hipLaunchKernelGGL(k_backbone_angles, dim3((unsigned)(((long long)B * nseg + 63) / 64)), dim3(64), 0, (hipStream_t)stream, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_rama_bin(void* stream, const float* angles, int F, const uint8_t* row_mask, int nseg, const uint8_t* rama_class,
                                const uint8_t* link, int skip_ends, uint64_t* counts, uint64_t* sums) {
    if (F <= 0 || nseg <= 0) return 0;
    if (!angles || !rama_class || !link || !counts || (long long)F * nseg > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    vmd_rama_params_t p{angles, F, nseg, row_mask, rama_class, link, skip_ends, (unsigned long long*)counts, (unsigned long long*)sums};
    hipLaunchKernelGGL(k_rama_bin, dim3((unsigned)(((long long)F * nseg + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t vmd_hip_ss_scratch_words(int B, int nseg) {
    if (B <= 0 || nseg <= 0) return 0;
    return 4 * (size_t)B * (size_t)nseg * (size_t)((nseg + 63) / 64);
}

// the three launches of a secondary-structure batch share one parameter block; every index a kernel forms is checked here, once
static int vmd_ss_params(vmd_ss_params_t* p, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags,
                         int B, int nseg, const int32_t* n, const int32_t* ca, const int32_t* c, const int32_t* o, const int32_t* rng,
                         const uint8_t* pro, const uint64_t* nbmask, uint64_t* scratch) {
    if (!xyz || !boxes || !n || !ca || !c || !o || !rng || !pro || !nbmask || !scratch || nseg > VMD_SS_SEG_MAX) return (int)hipErrorInvalidValue;
    const long long W = (nseg + 63) / 64;
    if ((long long)B * nseg * W > 0x7fffffffLL || (long long)B * W * W > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    const size_t rows = (size_t)B * (size_t)nseg * (size_t)W;
    unsigned long long* s = (unsigned long long*)scratch;
    *p = vmd_ss_params_t{vmd_frames(xyz, frame_stride, row_stride, boxes, pbc_flags, B), n, ca, c, o, rng, pro, (const unsigned long long*)nbmask,
                         nseg, (int)W, s, s + rows, s + 2 * rows, s + 3 * rows, nullptr, nullptr};
    return 0;
}

extern "C" int vmd_hip_ss_hbond(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags,
                                int B, int nseg, const int32_t* n, const int32_t* ca, const int32_t* c, const int32_t* o, const int32_t* rng,
                                const uint8_t* pro, const uint64_t* nbmask, uint64_t* scratch) {
    if (B <= 0 || nseg <= 0) return 0;
    vmd_ss_params_t p;
    if (int rc = vmd_ss_params(&p, xyz, frame_stride, row_stride, boxes, pbc_flags, B, nseg, n, ca, c, o, rng, pro, nbmask, scratch)) return rc;
    hipLaunchKernelGGL(k_ss_hbond, dim3((unsigned)((long long)B * p.W * p.W)), dim3(64), 0, (hipStream_t)stream, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_ss_bridges(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags,
                                  int B, int nseg, const int32_t* n, const int32_t* ca, const int32_t* c, const int32_t* o, const int32_t* rng,
                                  const uint8_t* pro, const uint64_t* nbmask, uint64_t* scratch) {
    if (B <= 0 || nseg <= 0) return 0;
    vmd_ss_params_t p;
    if (int rc = vmd_ss_params(&p, xyz, frame_stride, row_stride, boxes, pbc_flags, B, nseg, n, ca, c, o, rng, pro, nbmask, scratch)) return rc;
    hipLaunchKernelGGL(k_ss_bridges, dim3((unsigned)(((long long)B * nseg * p.W + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_ss_assign(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags,
                                 int B, int nseg, const int32_t* n, const int32_t* ca, const int32_t* c, const int32_t* o, const int32_t* rng,
                                 const uint8_t* pro, const uint64_t* nbmask, uint64_t* scratch, float* cls, float* pop) {
    if (B <= 0 || nseg <= 0) return 0;
    vmd_ss_params_t p;
    if (int rc = vmd_ss_params(&p, xyz, frame_stride, row_stride, boxes, pbc_flags, B, nseg, n, ca, c, o, rng, pro, nbmask, scratch)) return rc;
    if (!cls || !pop) return (int)hipErrorInvalidValue;
    p.cls = cls; p.pop = pop;
    hipLaunchKernelGGL(k_ss_assign, dim3((unsigned)B), dim3(256), 3 * (size_t)((nseg + 15) & ~15), (hipStream_t)stream, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

// the grid of a _small kernel: one wave per (frame, context)
static dim3 vmd_set_small_grid(long long BP) { return dim3((unsigned)((BP + VMD_SET_WAVES - 1) / VMD_SET_WAVES)); }

extern "C" size_t vmd_hip_shape_partial_doubles(int B, int P, int max_set) {
    if (B <= 0 || P <= 0 || max_set <= VMD_SET_WAVE_SET) return 0;
    return (size_t)B * (size_t)P * (size_t)vmd_set_chunks(max_set) * 10;
}

extern "C" int vmd_hip_shape(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                             const float* boxes, uint32_t pbc_flags, int B, int P,
                             const int32_t* set, const float* mass, const int32_t* offsets, int max_set,
                             double* partial, float* lin, float* plan, float* iso) {
    if (B <= 0 || P <= 0) return 0;
    if (!set || !mass || !offsets || !lin || !plan || !iso || max_set <= 0 || (long long)B * P > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    vmd_shape_params_t p{};
    p.f = vmd_frames(xyz, frame_stride, row_stride, boxes, pbc_flags, B); p.P = P;
    p.set = set; p.mass = mass; p.off = offsets; p.lin = lin; p.plan = plan; p.iso = iso;
    if (max_set <= VMD_SET_WAVE_SET) {
        hipLaunchKernelGGL(k_shape_small, vmd_set_small_grid((long long)B * P), dim3(VMD_SET_BLOCK), 0, (hipStream_t)stream, p);
        VMD_LAUNCH_CHECK();
        return 0;
    }
    p.nchunk = vmd_set_chunks(max_set);
    p.partial = partial;
    if (!partial || (long long)B * P * p.nchunk > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_shape_moments, dim3((unsigned)((long long)B * P * p.nchunk)), dim3(VMD_SET_BLOCK), 0, (hipStream_t)stream, p);
    VMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_shape_finish, dim3((unsigned)(((long long)B * P + 63) / 64)), dim3(64), 0, (hipStream_t)stream, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t vmd_hip_rmsd_workspace_bytes(int B, int P, int max_set) {
    if (B <= 0 || P <= 0 || max_set <= 0) return 0;
    if (max_set <= VMD_SET_WAVE_SET) return (size_t)B * (size_t)P * VMD_RMSD_NSUM * sizeof(double);      // one wave per set: the sums only
    const size_t blocks = (size_t)B * (size_t)P * (size_t)vmd_set_chunks(max_set);
    return blocks * (VMD_RMSD_NSUM * sizeof(double) + 4 * sizeof(int32_t));
}

// the parameter block of the rmsd and rmsf launches: the workspace holds the sums and, for the block kernels, the chunk shifts behind them
static int vmd_rmsd_params(vmd_rmsd_params_t& p, vmd_frames_t f, int P, const int32_t* set, const float* mass, const int32_t* offsets, int max_set,
                           const double* pose, const double* consts, int zero_row, void* workspace, float* out) {
    const long long BP = (long long)f.B * P;
    p = vmd_rmsd_params_t{};
    p.f = f; p.P = P; p.set = set; p.mass = mass; p.off = offsets;
    p.pose = const_cast<double*>(pose); p.cst = const_cast<double*>(consts);      // written by the pose pass only
    p.zero_row = zero_row; p.out = out;
    p.nchunk = vmd_set_chunks(max_set);
    if (!workspace || BP * p.nchunk > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    p.partial = (double*)workspace;
    if (max_set > VMD_SET_WAVE_SET) p.shift = (int32_t*)((char*)workspace + (size_t)(BP * p.nchunk) * VMD_RMSD_NSUM * sizeof(double));
    return 0;
}
// the sums of every (frame, context): one wave per set, or the chunk shifts and the block kernel
template <bool POSE>
static int vmd_rmsd_sums(hipStream_t s, const vmd_rmsd_params_t& p, int max_set) {
    const long long BP = (long long)p.f.B * p.P;
    if (max_set <= VMD_SET_WAVE_SET) {
        hipLaunchKernelGGL(k_rmsd_small<POSE>, vmd_set_small_grid(BP), dim3(VMD_SET_BLOCK), 0, s, p);
        VMD_LAUNCH_CHECK();
    } else {
        const dim3 blocks((unsigned)(BP * p.nchunk));
        hipLaunchKernelGGL(k_rmsd_shift, blocks, dim3(VMD_SET_BLOCK), 0, s, p);
        VMD_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_rmsd_moments<POSE>, blocks, dim3(VMD_SET_BLOCK), 0, s, p);
        VMD_LAUNCH_CHECK();
    }
    return 0;
}
// both passes: POSE runs the kernels' POSE forms over one frame (B = 1, frame_stride 0, no zero row, no values)
template <bool POSE>
static int vmd_rmsd_launch(void* stream, vmd_frames_t f, int P, const int32_t* set, const float* mass, const int32_t* offsets, int max_set,
                           const double* pose, const double* consts, int zero_row, void* workspace, float* out) {
    hipStream_t s = (hipStream_t)stream;
    vmd_rmsd_params_t p;
    if (int rc = vmd_rmsd_params(p, f, P, set, mass, offsets, max_set, pose, consts, zero_row, workspace, out)) return rc;
    if (int rc = vmd_rmsd_sums<POSE>(s, p, max_set)) return rc;
    hipLaunchKernelGGL(k_rmsd_finish<POSE>, dim3((unsigned)(((long long)f.B * P + 63) / 64)), dim3(64), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_rmsd_pose(void* stream, const float* xyz, size_t row_stride, const float* box, uint32_t pbc_flags, int P,
                                 const int32_t* set, const float* mass, const int32_t* offsets, int max_set,
                                 void* workspace, double* pose, double* consts) {
    if (P <= 0) return 0;
    if (!xyz || !set || !mass || !offsets || !pose || !consts || max_set <= 0) return (int)hipErrorInvalidValue;
    return vmd_rmsd_launch<true>(stream, vmd_frames(xyz, 0, row_stride, box, pbc_flags, 1), P, set, mass, offsets, max_set, pose, consts, -1,
                                 workspace, nullptr);
}

extern "C" int vmd_hip_rmsd(void* stream, const float* xyz, size_t frame_stride, size_t row_stride,
                            const float* boxes, uint32_t pbc_flags, int B, int P,
                            const int32_t* set, const float* mass, const int32_t* offsets, int max_set,
                            const double* pose, const double* consts, int zero_row, void* workspace, float* out) {
    if (B <= 0 || P <= 0) return 0;
    if (!xyz || !set || !mass || !offsets || !pose || !consts || !out || max_set <= 0 || (long long)B * P > 0x7fffffffLL)
        return (int)hipErrorInvalidValue;
    return vmd_rmsd_launch<false>(stream, vmd_frames(xyz, frame_stride, row_stride, boxes, pbc_flags, B), P, set, mass, offsets, max_set, pose,
                                  consts, zero_row, workspace, out);
}

// rmsf.  vmd_hip_rmsf_fit: the sums of the batch (have_sums != 0: an rmsd launch over the same sets has left them in
// `workspace`) and the rotation and centroids of every (frame, context) into rot.  vmd_hip_rmsf_accumulate: frames [b0, b0 + nb) of the
// batch into the record acc, in `groups` frame groups (<= 0: chosen here so that a small set still fills the card)
extern "C" size_t vmd_hip_rmsf_rot_doubles(int B, int P) { return B > 0 && P > 0 ? (size_t)B * (size_t)P * VMD_RMSF_NROT : 0; }

static int vmd_rmsf_params(vmd_rmsf_params_t& q, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags,
                           int B, int P, const int32_t* set, const float* mass, const int32_t* offsets, int max_set, const double* pose,
                           const double* consts, int zero_row, void* workspace, double* rot) {
    if (!xyz || !set || !mass || !offsets || !pose || !consts || !rot || max_set <= 0 || (long long)B * P > 0x7fffffffLL)
        return (int)hipErrorInvalidValue;
    q = vmd_rmsf_params_t{};
    q.rot = rot;
    return vmd_rmsd_params(q.r, vmd_frames(xyz, frame_stride, row_stride, boxes, pbc_flags, B), P, set, mass, offsets, max_set, pose, consts,
                           zero_row, workspace, nullptr);
}

extern "C" int vmd_hip_rmsf_fit(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes, uint32_t pbc_flags,
                                int B, int P, const int32_t* set, const float* mass, const int32_t* offsets, int max_set, const double* pose,
                                const double* consts, void* workspace, int have_sums, double* rot) {
    if (B <= 0 || P <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    vmd_rmsf_params_t q;
    if (int rc = vmd_rmsf_params(q, xyz, frame_stride, row_stride, boxes, pbc_flags, B, P, set, mass, offsets, max_set, pose, consts, -1, workspace,
                                 rot)) return rc;
    if (!have_sums) if (int rc = vmd_rmsd_sums<false>(s, q.r, max_set)) return rc;
    hipLaunchKernelGGL(k_rmsf_rotation, dim3((unsigned)(((long long)B * P + 63) / 64)), dim3(64), 0, s, q);
    VMD_LAUNCH_CHECK();
    return 0;
}

// the frame groups of one accumulate launch.  Block kernel: about four blocks per CU of (context, chunk, group), never more than
// VMD_RMSF_FRAMES frames to a group; one wave per set: about 4096 waves.  `want` > 0 asks for that many (clamped the same way)
extern "C" int vmd_hip_rmsf_groups(int nb, int P, int max_set, int want) {
    if (nb <= 0 || P <= 0 || max_set <= 0) return 0;
    const bool small = max_set <= VMD_SET_WAVE_SET;
    const long long units = small ? P : (long long)P * vmd_set_chunks(max_set);
    long long g = want > 0 ? want : ((small ? 4096 : 1024) + units - 1) / units;
    const long long lo = small ? 1 : (nb + VMD_RMSF_FRAMES - 1) / VMD_RMSF_FRAMES;
    g = g < lo ? lo : g;
    g = g > nb ? nb : g;
    return (int)g;
}

extern "C" int vmd_hip_rmsf_accumulate(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes,
                                       uint32_t pbc_flags, int B, int P, const int32_t* set, const float* mass, const int32_t* offsets,
                                       int max_set, const double* pose, const double* consts, int zero_row, void* workspace,
                                       const double* rot, int b0, int nb, int groups, uint64_t* acc) {
    if (B <= 0 || P <= 0 || nb <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    vmd_rmsf_params_t q;
    if (int rc = vmd_rmsf_params(q, xyz, frame_stride, row_stride, boxes, pbc_flags, B, P, set, mass, offsets, max_set, pose, consts, zero_row,
                                 workspace, const_cast<double*>(rot))) return rc;
    if (!acc || b0 < 0 || b0 + (long long)nb > B) return (int)hipErrorInvalidValue;
    q.acc = acc; q.b0 = b0; q.nb = nb;
    q.groups = vmd_hip_rmsf_groups(nb, P, max_set, groups);
    if (max_set <= VMD_SET_WAVE_SET) {
        if ((long long)P * q.groups > 0x7fffffffLL) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL(k_rmsf_small, vmd_set_small_grid((long long)P * q.groups), dim3(VMD_SET_BLOCK), 0, s, q);
    } else {
        const long long blocks = (long long)P * q.r.nchunk * q.groups;
        if (blocks > 0x7fffffffLL || (nb + q.groups - 1) / q.groups > VMD_RMSF_FRAMES) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL(k_rmsf_accumulate, dim3((unsigned)blocks), dim3(VMD_SET_BLOCK), 0, s, q);
    }
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_bbox(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, int B, int natoms, float* out) {
    if (B <= 0 || natoms <= 0) return 0;
    hipLaunchKernelGGL(k_bbox, dim3(B), dim3(1024), 0, (hipStream_t)stream, xyz, frame_stride, row_stride, natoms, out);
    VMD_LAUNCH_CHECK();
    return 0;
}

// ---- two-level cell build (k_cells_bin / k_cells_pen_scan / k_cells_pen_sort) --------------------------------------------------
#define VMD_PEN_MAX 4096            // pencils per frame the LDS table of k_cells_bin holds
#define VMD_PEN_CAP_MAX 8192        // atoms of one pencil k_cells_pen_sort stages through LDS (96 KB)
static int g_cells_pencil = 1;
extern "C" int vmd_hip_set_cells_pencil(int on) { const int old = g_cells_pencil; g_cells_pencil = on; return old; }
extern "C" int vmd_hip_cells_pencil_ok(vmd_grid_t grid) {
    return g_cells_pencil && (long long)grid.ny * grid.nz <= VMD_PEN_MAX && grid.nxf <= 8192;
}
extern "C" int vmd_hip_cells_pencil_cap_max(void) { return VMD_PEN_CAP_MAX; }

static int g_cells_bin_lds = 1;   // level 1 orders a block's records by pencil in LDS before writing them (A/B switch)
extern "C" int vmd_hip_set_cells_bin_lds(int on) { const int old = g_cells_bin_lds; g_cells_bin_lds = on ? 1 : 0; return old; }
static thread_local uint32_t g_cells_overflow_bit = 1u;    // per host thread, set by the evaluator before each selection's build (vmd_hip_set_cells_overflow_bit)
extern "C" uint32_t vmd_hip_set_cells_overflow_bit(uint32_t bit) { const uint32_t old = g_cells_overflow_bit; g_cells_overflow_bit = bit ? bit : 1u; return old; }
static int g_cells_rec3 = 1;      // 12-byte bucket records where the cell kind allows it (A/B switch)
extern "C" int vmd_hip_set_cells_rec3(int on) { const int old = g_cells_rec3; g_cells_rec3 = on ? 1 : 0; return old; }

// level 1's parameters, for the counting mode (no buckets: pen_off, bucket and overflow NULL) and for the build; the thread's overflow bit
static vmd_bin_params_t vmd_bin_params(const vmd_cells_params_t& c, const uint32_t* pen_off, uint32_t* pen_count, float* bucket, uint32_t* overflow,
                                       int total_cap, int rec3) {
    vmd_bin_params_t q = {};
    q.c = c; q.pen_off = pen_off; q.pen_count = pen_count; q.bucket = bucket; q.overflow = overflow; q.overflow_bit = g_cells_overflow_bit;
    q.npen = c.grid.ny * c.grid.nz; q.total_cap = total_cap; q.rec3 = rec3;
    return q;
}
static dim3 vmd_bin_grid(int nsel, int frames) { return dim3((nsel + 1024 * VMD_BIN_ILP - 1) / (1024 * VMD_BIN_ILP), frames); }   // level 1

extern "C" int vmd_hip_cells_pencil_count(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes,
                                          uint32_t pbc_flags, int S, const int32_t* sel, int nsel, vmd_grid_t grid, uint32_t* counts) {
    hipStream_t s = (hipStream_t)stream;
    if (S <= 0 || nsel <= 0) return 0;
    const int npen = grid.ny * grid.nz;
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(uint32_t) * (size_t)S * npen, s);
    if (e != hipSuccess) return (int)e;
    const vmd_bin_params_t q = vmd_bin_params(vmd_cells_params(xyz, frame_stride, row_stride, boxes, pbc_flags, sel, nsel, 0, grid),
                                              nullptr, counts, nullptr, nullptr, 0, 0);
    hipLaunchKernelGGL(k_cells_bin, vmd_bin_grid(nsel, S), dim3(1024), sizeof(uint32_t) * npen, s, q);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_cells_build_pencil(void* stream, const float* xyz, size_t frame_stride, size_t row_stride, const float* boxes,
                                          uint32_t pbc_flags, int B, const int32_t* sel, int nsel, int nsel_pad, vmd_grid_t grid,
                                          const uint32_t* pen_off, int total_cap, int cap_max, uint32_t* pen_count, uint32_t* pen_start,
                                          float* bucket, uint32_t* overflow, uint32_t* cell_start, float* sorted) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0 || nsel <= 0) return 0;
    const int npen = grid.ny * grid.nz;
    if (!vmd_hip_cells_pencil_ok(grid) || cap_max > VMD_PEN_CAP_MAX) return (int)hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(pen_count, 0, sizeof(uint32_t) * (size_t)B * npen, s);
    if (e != hipSuccess) return (int)e;
    // x-periodic, non-triclinic cells: the grid bins the wrapped x itself, so the record need not carry the fine cell
    const int rec3 = (g_cells_rec3 && (pbc_flags & 1u) && !(pbc_flags & VMD_PBC_TRICLINIC)) ? 1 : 0;
    const vmd_bin_params_t q = vmd_bin_params(vmd_cells_params(xyz, frame_stride, row_stride, boxes, pbc_flags, sel, nsel, nsel_pad, grid),
                                              pen_off, pen_count, bucket, overflow, total_cap, rec3);
    const size_t shm_sorted = sizeof(uint32_t) * (3 * (size_t)npen + 1040 + (size_t)1024 * VMD_BIN_ILP * (rec3 ? 4 : 5));
    if (g_cells_bin_lds && shm_sorted <= VMD_LDS_OPT_IN) {
        int eb = vmd_lds_opt_in((const void*)k_cells_bin_sorted);
        if (eb) return eb;
        hipLaunchKernelGGL(k_cells_bin_sorted, vmd_bin_grid(nsel, B), dim3(1024), shm_sorted, s, q);
    } else {
        hipLaunchKernelGGL(k_cells_bin, vmd_bin_grid(nsel, B), dim3(1024), sizeof(uint32_t) * npen, s, q);
    }
    VMD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cells_pen_scan, dim3(B), dim3(256), 0, s, (const uint32_t*)pen_count, pen_off, pen_start, npen);
    VMD_LAUNCH_CHECK();
    vmd_pensort_params_t ps{bucket, pen_off, pen_count, pen_start, cell_start, sorted, npen, grid.nxf, grid.ncell, nsel_pad, total_cap, cap_max, boxes, rec3};
    const size_t shm = sizeof(uint32_t) * ((size_t)grid.nxf + 256 + 3 * (size_t)cap_max);
    if (shm > VMD_LDS_OPT_IN) return (int)hipErrorInvalidValue;
    int ea = vmd_lds_opt_in((const void*)k_cells_pen_sort);
    if (ea) return ea;
    // grid.y = B <= 65535 (frame batches are far smaller); pencils on grid.x
    hipLaunchKernelGGL(k_cells_pen_sort, dim3(npen, B), dim3(256), shm, s, ps);
    VMD_LAUNCH_CHECK();
    return 0;
}

// dst[i] += mult * src[i] (u64): one pair pass feeding several histograms (class decomposition of co-evaluated RDFs)
__global__ __launch_bounds__(256) void k_axpy_u64(uint64_t* __restrict__ dst, const uint64_t* __restrict__ src, size_t n, uint64_t mult,
                                                  const uint32_t* __restrict__ skip) {
    if (skip && *skip) return;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const uint64_t v = src[i]; if (v) dst[i] += mult * v; }
}
extern "C" int vmd_hip_axpy_u64(void* stream, uint64_t* dst, const uint64_t* src, size_t n, uint64_t mult, const uint32_t* skip_flag) {
    if (n == 0 || mult == 0) return 0;
    hipLaunchKernelGGL(k_axpy_u64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dst, src, n, mult, skip_flag);
    VMD_LAUNCH_CHECK();
    return 0;
}

// dst[i] += src[i]: merges one frame block's partial accumulator into another (block partials, filtered evaluation)
__global__ __launch_bounds__(256) void k_add_u64(uint64_t* __restrict__ dst, const uint64_t* __restrict__ src, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const uint64_t v = src[i]; if (v) dst[i] += v; }
}
extern "C" int vmd_hip_add_u64(void* stream, uint64_t* dst, const uint64_t* src, size_t n) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_add_u64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dst, src, n);
    VMD_LAUNCH_CHECK();
    return 0;
}

// counts[index] += value: the self pairs (d = 0) a half-shell pass never visits, when the closed interval counts them
// An empty kernel with a name of its own: bench.py launches it where its timed region begins, so that a counter collection of the same
// command (scripts/pmc_traffic.py) can tell the steady-state dispatches from the warm-up's (capacity sampling, first-touch, overflow repeats)
__global__ void k_marker_timed_region() {}
extern "C" int vmd_hip_marker(void* stream) {
    hipLaunchKernelGGL(k_marker_timed_region, dim3(1), dim3(64), 0, (hipStream_t)stream);
    VMD_LAUNCH_CHECK();
    return 0;
}
__global__ void k_bump_u64(uint64_t* p, uint64_t v) { if (threadIdx.x == 0 && blockIdx.x == 0) *p += v; }
extern "C" int vmd_hip_bump_u64(void* stream, uint64_t* p, uint64_t v) {
    hipLaunchKernelGGL(k_bump_u64, dim3(1), dim3(64), 0, (hipStream_t)stream, p, v);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_counts_to_float(void* stream, const uint64_t* counts, size_t n, float* values, float* max_out, float scale) {
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) return 0;
    if (max_out) {
        hipError_t e = hipMemsetAsync(max_out, 0, sizeof(float), s);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k_counts_to_float, dim3((unsigned)((n + 2047) / 2048)), dim3(256), 0, s, counts, n, values, (unsigned*)max_out, scale);
    VMD_LAUNCH_CHECK();
    return 0;
}

extern "C" int vmd_hip_synth_frames(void* stream, float* xyz, size_t frame_stride, size_t row_stride, int B, uint32_t frame0,
                                    uint64_t seed, uint32_t n_atoms, uint32_t n_blob, float L, float sigma) {
    hipStream_t s = (hipStream_t)stream;
    if (B <= 0 || n_atoms <= n_blob) return 0;
    vmd_synth_params_t p{xyz, frame_stride, row_stride, B, frame0, seed, n_atoms, n_blob, L, sigma};
    hipLaunchKernelGGL(k_synth, dim3((n_atoms - n_blob + 255) / 256, B), dim3(256), 0, s, p);
    VMD_LAUNCH_CHECK();
    return 0;
}
