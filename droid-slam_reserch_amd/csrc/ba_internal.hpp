// ba_internal.hpp -- workspace layout of one `ba` call, shared by the host API and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace droid {

constexpr int LIN_THREADS = 256;
constexpr int LIN_PPT = 2;                       // pixels per thread per chunk
constexpr int LIN_CP = LIN_THREADS * LIN_PPT;    // pixels per workgroup chunk
constexpr int LIN_WAVES = LIN_THREADS / 64;      // waves per workgroup: each leaves its own partial sums of a chunk
constexpr int CHOL_NB = 64;                      // Cholesky block size
// row pitch of the augmented system in doubles: 128-byte rows, so 64-column tiles never share a cache line
__host__ __device__ inline int chol_ld(int n) { return (n + 1 + 15) & ~15; }
// ints of hand-off flags (done[block rows], dver[block rows], abort) of an n x n solve; what they mean: cfp_input (chol.hip)
__host__ __device__ inline size_t chol_flag_words(int n) { return 2 * ((size_t)(n + 1 + CHOL_NB - 1) / CHOL_NB) + 8; }
// lower-triangle tiles of the augmented system in column-major order: tile (bi, bj), bi >= bj.  The same index is the
// tile's owner (index mod grid) under both schedulers of the single-launch factorisation and its hand-over slot
__host__ __device__ inline int chol_tile_index(int nrb, int bi, int bj) { return bj * nrb - bj * (bj - 1) / 2 + (bi - bj); }
__host__ __device__ inline size_t chol_tiles(int n) {
  const int nb = (n + CHOL_NB - 1) / CHOL_NB, nrb = (n + 1 + CHOL_NB - 1) / CHOL_NB;
  return (size_t)chol_tile_index(nrb, nb, nb);  // = sum_{j<nb} (nrb - j)
}
// `ldiag` scratch of the single-launch factorisation, in 64x64 tiles:
//   [nb]         factored diagonal tiles L_jj (+ the inverses of their 16x16 diagonal blocks in the upper part),
//   [nb]         M_j = L[j+1,j] L_jj^-1 (the back-substitution multiplies by them instead of solving),
//   [chol_tiles] hand-over slots `lfin` of the final panel tiles (data-tagged: preset to 0xFF bytes, a 16-column
//                strip is there when its bytes are not)
__host__ __device__ inline size_t chol_mbuf_offset(int n) { return ((size_t)(n + CHOL_NB - 1) / CHOL_NB) * CHOL_NB * CHOL_NB; }
__host__ __device__ inline size_t chol_lfin_offset(int n) { return 2 * chol_mbuf_offset(n); }
__host__ __device__ inline size_t chol_ldiag_doubles(int n) { return chol_lfin_offset(n) + chol_tiles(n) * CHOL_NB * CHOL_NB; }
// Back-substitution after a single-launch factorisation: workgroup J owns the block columns 2J and 2J+1 (the top one
// a single column when their number is odd); x crosses a workgroup boundary once per pair.
__host__ __device__ inline int chol_bs_pairs_grid(int nb) { return (nb + 1) / 2; }
__host__ __device__ inline int chol_bs_pairs_owner(int col) { return col / 2; }
__host__ __device__ inline int chol_bs_pairs_first(int wg) { return 2 * wg; }

// Packed lower triangle + rhs row, BLOCK-COLUMN major (what the ranks all-reduce): block column J = columns
// 64 J .. 64 J + w_J - 1 (w_J = 64, the last one n - 64 J) holds rows 64 J .. n (row n = rhs) as rows of w_J doubles.
// The factorisation consumes block columns left to right, so a PREFIX of this tensor is all its first block columns
// need: the collective can be cut into column chunks that arrive in the order the solver wants them (overlap mode).
// (The strict upper halves of the diagonal tiles are carried along as zeros: 4 % of the bytes.)
__host__ __device__ inline size_t pk_colbase(int n, int J) {
  return (size_t)CHOL_NB * ((size_t)J * (size_t)(n + 1) - (size_t)CHOL_NB * (size_t)J * (size_t)(J - 1) / 2);
}
__host__ __device__ inline int pk_width(int n, int J) { return (n - CHOL_NB * J) < CHOL_NB ? (n - CHOL_NB * J) : CHOL_NB; }
__host__ __device__ inline size_t pk_total(int n) {
  if (n <= 0) return 0;
  const int nb = (n + CHOL_NB - 1) / CHOL_NB;
  return pk_colbase(n, nb - 1) + (size_t)(n + 1 - CHOL_NB * (nb - 1)) * (size_t)pk_width(n, nb - 1);
}
__host__ __device__ inline size_t pk_index(int n, int gi, int gj) {   // gi >= 64 (gj / 64); gi = n: rhs row
  const int J = gj / CHOL_NB;
  return pk_colbase(n, J) + (size_t)(gi - CHOL_NB * J) * (size_t)pk_width(n, J) + (size_t)(gj - CHOL_NB * J);
}
// the same in 32-bit arithmetic for the kernels' atomics (the packed tensor has < 2^31 elements up to n = 65 000)
__host__ __device__ inline unsigned pk_index32(int n, int gi, int gj) {
  const int J = gj >> 6, c0 = J << 6;
  const int w = (n - c0) < CHOL_NB ? (n - c0) : CHOL_NB;
  return (unsigned)(CHOL_NB * (J * (n + 1) - (CHOL_NB / 2) * J * (J - 1)) + (gi - c0) * w + (gj - c0));
}

enum { HDR_STATUS = 0, HDR_M = 1, HDR_CHOL_FAIL = 2, HDR_NENT = 3, HDR_NWORK = 4,
       HDR_NC1 = 5, HDR_NC2 = 6,  // slots served by the two SYRK variants (classes 1, 2)
       HDR_WORDS = 16 };
enum { STATUS_BAD_INDEX = 1, STATUS_ETA_ROWS = 2, STATUS_CHOL_FAIL = 4, STATUS_CHOL_STALL = 8 };

// Plain-old-data view of the workspace, passed to kernels by value.
struct BaView {
  int E, nbuf, H, W, HW;
  int t0, t1, P, M;        // window, poses in it, depth slots the host sized the buffers for
  int n, ld;               // n = 6P unknowns; system is (n+1) x ld, ld = roundup16(n+1) (128-byte rows), row n = rhs
  int nch;                 // pixel chunks of the linearisation kernel
  int own0, own1;          // frames whose depth this rank owns
  int motion_only;         // prep: validate indices only, no depth slots
  int* hdr;                // [HDR_WORDS] status, slot count, ...
  int* slot_of;            // [nbuf] frame -> depth slot or -1
  int* kx;                 // [nbuf] slot -> frame (sorted)
  int* seg_ptr;            // [nbuf+1] CSR of edges by slot
  int* seg_edge;           // [E]
  int* cursor;             // [nbuf+1] scratch
  int* ent_ptr;            // [nbuf+1] CSR of Schur entries by slot
  int* ent_row;            // [M+E] row of Erows
  int* ent_pose;           // [M+E] pose index in the window
  int* wk_ptr;             // [nbuf+1] scratch (slot sizes while sorting)
  int* order;              // [nbuf+1] slots sorted by descending edge count: big slots are dispatched first
  int* xtmp;               // [3(E+1)] prep scratch: unsorted segment fill, window flag and slot of every sorted position
  int* cls_list;           // [2][nbuf+2] the slots of SYRK class 1 / class 2, ascending (ba_syrk3_kernel)
  int* gt_ptr;             // [nbuf+2] first partial-sum tile of a slot served by ba_schur2_kernel (exclusive scan)
  double* Gpart;           // [tiles][s2_split][256] fp64 partial sums of those slots' Gram tiles, one per pixel range
  int s2_split;            // pixel ranges per slot of ba_schur2_kernel
  float* Hpart;            // [E][nch][LIN_WAVES][32] per-(edge, chunk, wave of the chunk's workgroup) partial Hjj (21) + vj (6),
                           // words 27..31 zero; the assemble step adds the waves of a chunk in fp32, the chunks in fp64
  float* Q;                // [M][HW] 1/C
  float* w;                // [M][HW]
  float* Erows;            // unused (nullptr): sparse slots recompute their E rows where they are consumed
  float* Ebuf;             // dense graphs only (`wide`): unscaled E rows, 6*(M+E)*HW floats, per slot tiled by 32-pixel stage
                           // (ba_kernels.hip::ebuf_index), written by the linearisation and consumed by the SYRK-only Schur kernels
  float* sy_part[2];       // dense graphs: fp32 tiles of S per (slot of SYRK class 1 / 2, pixel range), summed by ba_syrk_fold_kernel
  int sy_ns[2];            // pixel splits (grid y) of the two SYRK launches
  int wide;                // host decision: mean out-degree >= 12 (dense global BA, edge-sharded ranks)
  int zsplit;              // linearisation: workgroups per (slot, pixel chunk), each takes a range of the slot's edges
  float* zpart;            // zsplit > 1: [zsplit][M][8][HW] partial C, w and self-row sums of those workgroups
  double* sys;             // [n+1][ld] reduced camera system, lower triangle, row n = rhs
  double* psys;            // the same entries packed block-column major (pk_index): what a rank's build phase
                           // accumulates into when the systems are all-reduced
  int packed;              // 1: the build kernels add into psys (multi-GPU), 0: straight into sys
  double* xsol;            // [ld] solve scratch / solution
  float* dx;               // [P][6]
  int* bs_flags;           // [chol_flag_words(n)] hand-off flags of the single-launch factorisation
  double* ldiag;           // [ceil(n/64)][64][64] factored diagonal tiles, then the hand-over slots of the panel tiles
  int* hint;               // host-side launch hints (droid_ba_attach_launch_hints): 2 ints of page-locked host memory {tag, slots of
                           // Schur class 3}, written by ba_prep_kernel; nullptr: none.  hint_tag = tag of this workspace's last prepare
  int hint_tag;
  int* ov_ready;           // [block columns of the system] overlap mode: epoch of the last iteration whose reduced columns are in `sys`
  float* pose_snap;        // [nbuf][7] the poses the iteration was linearised at: written by a spare workgroup of the depth-slot
                           // linearisation launch, read by ba_backsub_kernel, whose last workgroup retracts the caller's tensor
};

// Launch geometry of one iteration.  ba_carve sizes buffers with these numbers and ba_launch_plan (below) turns them into
// grids: nothing else on the host decides a grid of the build phase.
constexpr int SY_WGS = 1024;  // (slot, pixel range) workgroups of the class-1 SYRK launch: four per CU balance the uneven slots (A/B 512 / 768 / 1024 / 1536 / 2048: 270 / 265 / 253 / 262 / 270 us at 256 slots)
constexpr int S2_WGS = 1536;  // (slot, pixel range) workgroups of the sparse Schur launch
constexpr int SF_WGS = 1536;  // (slot, pixel range) workgroups of the block-pair Schur launch
constexpr int LIN_WGS = 1536; // (slot, pixel chunk, edge range) workgroups of the linearisation launch
constexpr int LIN_ZERO_WGS = 192;  // workgroups of the linearisation launch that clear the system instead
constexpr int SF_TP = 64;     // pixels per LDS tile of the block-pair Schur kernel; 4 threads per pixel split the edges
// Dense slots (more than 16 entries) are served by the SYRK-only kernels.
constexpr int SW_MID = 256;   // rows (incl. the w row) served by the two-workgroups-per-CU variant (42 entries; two staging rounds of 128 rows)
constexpr int SW_BIG = 512;   // rows served by the one-per-CU variant (85 entries)
constexpr int tri_tiles16(int rows) { return (rows / 16) * (rows / 16 + 1) / 2; }
constexpr int SY_T1 = tri_tiles16(SW_MID), SY_T2 = tri_tiles16(SW_BIG);  // 16x16 tiles (1 KB of fp32 each) of a class-1 / class-2 slot's lower triangle: 136 / 528
constexpr int SY_FOLD_GROUPS = SY_T1 / 4;  // grid y of the SYRK fold: four waves per workgroup, one class-1 tile per wave

// Carves `ws` (may be null: size query only) into the view.  Host-only arithmetic.
inline size_t ba_carve(BaView& v, void* ws, int E, int nbuf, int H, int W, int t0, int t1, int M) {
  v.E = E; v.nbuf = nbuf; v.H = H; v.W = W; v.HW = H * W;
  v.t0 = t0; v.t1 = t1; v.P = t1 - t0; v.M = M;
  v.n = 6 * v.P; v.ld = chol_ld(v.n);
  v.nch = (v.HW + LIN_CP - 1) / LIN_CP;
  v.own0 = 0; v.own1 = nbuf; v.motion_only = 0;
  v.hint = nullptr; v.hint_tag = 0;
  size_t off = 0;
  char* base = static_cast<char*>(ws);
  auto take = [&](size_t bytes) {
    void* p = base ? base + off : nullptr;
    off += (bytes + 255) & ~size_t(255);
    return p;
  };
  v.hdr = static_cast<int*>(take(sizeof(int) * HDR_WORDS));
  v.slot_of = static_cast<int*>(take(sizeof(int) * (nbuf + 1)));
  v.kx = static_cast<int*>(take(sizeof(int) * (nbuf + 1)));
  v.seg_ptr = static_cast<int*>(take(sizeof(int) * (nbuf + 2)));
  v.seg_edge = static_cast<int*>(take(sizeof(int) * (E + 1)));
  v.cursor = static_cast<int*>(take(sizeof(int) * (nbuf + 2)));
  v.ent_ptr = static_cast<int*>(take(sizeof(int) * (nbuf + 2)));
  v.ent_row = static_cast<int*>(take(sizeof(int) * ((size_t)M + E + 1)));
  v.ent_pose = static_cast<int*>(take(sizeof(int) * ((size_t)M + E + 1)));
  v.wk_ptr = static_cast<int*>(take(sizeof(int) * (nbuf + 2)));
  v.order = static_cast<int*>(take(sizeof(int) * (nbuf + 2)));
  v.gt_ptr = static_cast<int*>(take(sizeof(int) * (nbuf + 2)));
  v.cls_list = static_cast<int*>(take(sizeof(int) * 2 * (nbuf + 2)));
  v.xtmp = static_cast<int*>(take(sizeof(int) * 3 * ((size_t)E + 1)));
  v.Hpart = static_cast<float*>(take(sizeof(float) * ((size_t)E * v.nch * LIN_WAVES * 32 + 32)));
  v.Q = static_cast<float*>(take(sizeof(float) * ((size_t)M * v.HW + 4)));
  v.w = static_cast<float*>(take(sizeof(float) * ((size_t)M * v.HW + 4)));
  v.Erows = nullptr;  // E rows are recomputed where they are consumed, never stored ...
  v.wide = (M > 0 && (long)E >= 12l * M && (v.HW % 32) == 0) ? 1 : 0;
  v.Ebuf = nullptr;   // ... except for dense graphs, where the recomputation would be repeated per output share
  if (v.wide) v.Ebuf = static_cast<float*>(take(sizeof(float) * (6 * ((size_t)M + E) * v.HW + 64)));
  v.sy_part[0] = v.sy_part[1] = nullptr;
  v.sy_ns[0] = v.sy_ns[1] = 0;
  if (v.wide) {
    // pixel splits of the SYRK launches: enough (slot, range) workgroups to fill 256 CUs four times over (class 1: one 12-wave workgroup per
    // CU; class 2: four shares per pair); a split costs a set of partial tiles, no atomics.  A launch has M * ns pairs at most:
    // SY_T1 (class 1: <= SW_MID rows) or SY_T2 (class 2: <= SW_BIG rows) tiles of 1 KB each
    const int stages = v.HW / 32;
    int nsw = (SY_WGS + M - 1) / M, nsb = (256 + 4 * M - 1) / (4 * M);
    nsw = nsw < 2 ? 2 : (nsw > stages ? stages : nsw);
    nsb = nsb < 2 ? 2 : (nsb > stages ? stages : nsb);
    if (nsw > 16) nsw = 16;  // SY_MAXSPLIT (ba_kernels.hip): the kernels never use more ranges per slot
    if (nsb > 16) nsb = 16;
    v.sy_ns[0] = nsw; v.sy_ns[1] = nsb;
    v.sy_part[0] = static_cast<float*>(take(sizeof(float) * ((size_t)M * nsw * SY_T1 * 256 + 64)));
    v.sy_part[1] = static_cast<float*>(take(sizeof(float) * ((size_t)M * nsb * SY_T2 * 256 + 64)));
  }
  // few depth slots (edge-sharded ranks, small windows): split every slot's edges over several
  // workgroups so that the linearisation still fills the chip
  v.zsplit = 1;
  if (M > 0) {
    const int z = LIN_WGS / (M * v.nch);
    v.zsplit = z < 1 ? 1 : (z > 8 ? 8 : z);
  }
  v.zpart = nullptr;
  if (v.zsplit > 1) v.zpart = static_cast<float*>(take(sizeof(float) * ((size_t)v.zsplit * M * 8 * v.HW + 64)));
  // Schur complement of sparse slots (<= S2_MAXE edges): every (slot, pixel range) workgroup leaves the fp64
  // Gram tiles of its E rows here; tiles(n edges) <= 1.75 n + 1 (7 row tiles of 16 at 16 edges)
  v.s2_split = 1;
  v.Gpart = nullptr;
  if (M > 0) {
    const int ptiles = (v.HW + 63) / 64;
    int ns = S2_WGS / M;
    v.s2_split = ns < 1 ? 1 : (ns > ptiles ? ptiles : ns);
    size_t tiles = (size_t)E * 7 / 4 + (size_t)M + 1;
    if (tiles > (size_t)28 * M) tiles = (size_t)28 * M;
    v.Gpart = static_cast<double*>(take(sizeof(double) * (tiles * v.s2_split * 256 + 64)));
  }
  v.sys = static_cast<double*>(take(sizeof(double) * ((size_t)(v.n + 1) * v.ld + 8)));
  v.psys = static_cast<double*>(take(sizeof(double) * (pk_total(v.n) + 8)));
  v.packed = 0;
  v.xsol = static_cast<double*>(take(sizeof(double) * ((size_t)v.ld + 1)));
  v.bs_flags = static_cast<int*>(take(sizeof(int) * chol_flag_words(v.n)));   // directly after xsol: one fill presets both
  v.ldiag = static_cast<double*>(take(sizeof(double) * chol_ldiag_doubles(v.n)));
  v.dx = static_cast<float*>(take(sizeof(float) * ((size_t)v.n + 8)));
  v.ov_ready = static_cast<int*>(take(sizeof(int) * ((size_t)(v.n + 1 + CHOL_NB - 1) / CHOL_NB + 8)));
  v.pose_snap = static_cast<float*>(take(sizeof(float) * 7 * (size_t)nbuf));
  return off;
}

// 4-byte words from xsol through the end of bs_flags (contiguous in the workspace): what one iteration's solve
// expects preset to 0xFF bytes.  With edges, the assemble kernel's spare workgroups do it (and zero the failure
// flag); without, launch_chol_preset's fills do.
__host__ __device__ inline int solver_preset_words(const BaView& v) {
  return (int)((reinterpret_cast<const char*>(v.bs_flags) - reinterpret_cast<const char*>(v.xsol)) / 4 +
               (long)chol_flag_words(v.n));
}
// 32 KB blocks of the panel-tile hand-over slots (ldiag + chol_lfin_offset), preset to 0xFF bytes the same way
__host__ __device__ inline int solver_preset_tiles(const BaView& v) { return v.n > 0 ? (int)chol_tiles(v.n) : 0; }

// Launch plan of one iteration's build phase: every grid size launch_build_stage uses that ba_carve has not already
// put into the view (zsplit, s2_split, sy_ns).  Host-only arithmetic.
struct BaLaunchPlan {
  int zero_wgs;       // workgroups of the linearisation launch that clear the system
  int asm_units;      // assemble units: one per edge + the presets of the solver scratch; 0 without edges
  dim3 schur2;        // grid of the sparse Schur launch: (slots + spare columns that take the assemble units, pixel ranges)
  int sf_split;       // pixel ranges per slot of the block-pair Schur launch
  dim3 syrk[2], fold; // grids of the two SYRK launches and of their fold (dense graphs only)
};
inline BaLaunchPlan ba_launch_plan(const BaView& v) {
  BaLaunchPlan p;
  p.zero_wgs = LIN_ZERO_WGS;
  p.asm_units = v.E > 0 ? v.E + (solver_preset_words(v) + 1023) / 1024 + solver_preset_tiles(v) : 0;
  p.schur2 = dim3(v.M + (p.asm_units + 4 * v.s2_split - 1) / (4 * v.s2_split), v.s2_split);
  // pixel split so that small graphs still fill the chip (atomics grow with the split)
  const int tiles = (v.HW + SF_TP - 1) / SF_TP, ns = SF_WGS / (v.M > 0 ? v.M : 1);
  p.sf_split = ns < 1 ? 1 : (ns > tiles ? tiles : ns);
  p.syrk[0] = dim3(v.M, v.sy_ns[0], 1);
  p.syrk[1] = dim3(v.M, v.sy_ns[1], 4);
  p.fold = dim3(v.M, SY_FOLD_GROUPS, 2);
  return p;
}

// What one Cholesky solve works on: the augmented system S ((n+1) x ld, row n = rhs, factored in place), the
// solution x [n], the scratch of the single-launch kernels (flags [chol_flag_words(n)], ldiag [chol_ldiag_doubles(n)])
// and the failure word (1: not positive definite, 2: stalled grid).  Every solve expects x, the flags and the
// hand-over slots of ldiag preset to 0xFF bytes and the failure word to 0: by launch_chol_preset, or in the BA by the
// assemble kernel (above).
struct CholSystem {
  double* S; int n, ld; double* x; int* flags; double* ldiag; int* fail;
  explicit CholSystem(const BaView& v)
      : S(v.sys), n(v.n), ld(v.ld), x(v.xsol), flags(v.bs_flags), ldiag(v.ldiag), fail(v.hdr + HDR_CHOL_FAIL) {}
  // droid_chol_solve: S, ldiag and the flags carved out of one scratch buffer of scratch_doubles(n) doubles
  CholSystem(double* scratch, int n, double* x, int* fail);
  static size_t scratch_doubles(int n);
};

// kernels' launchers (ba_kernels.hip / chol.hip)
// one wave through the linearisation's wave_reduce32: in [64][32] (lane, value) -> out [64] (what each lane returns)
void launch_wave_reduce32_test(const float* in, float* out, hipStream_t s);
// the linearisation (stage 0 of launch_build_stage) of a prepared workspace alone; ragged: with the per-lane guarded
// body of ba_lin_kernel also where the pixel count is a multiple of the chunk and the product runs the FULL body
void launch_lin_test(const BaView& v, const float* poses, const float* disps, const float* intr, const float* sens,
                     const float* targets, const float* weights, const float* eta, const int64_t* ii, const int64_t* jj,
                     bool motion_only, bool ragged, hipStream_t s);
void launch_prep(const BaView& v, const int64_t* ii, const int64_t* jj, hipStream_t s);
// multi-GPU: expand the (all-reduced) packed system into the pitched matrix the solver factors in place
void launch_unpack_system(const BaView& v, hipStream_t s);
// One stage of the build phase, launched as `plan` (ba_launch_plan of v) says: 0 memset+linearise, 1 assemble, 2 schur
void launch_build_stage(const BaView& v, const BaLaunchPlan& plan, const float* poses, const float* disps,
                        const float* intr, const float* sens, const float* targets, const float* weights,
                        const float* eta, const int64_t* ii, const int64_t* jj, bool motion_only,
                        int stage, hipStream_t s);
// status_mirror: optional device-visible host words {status, depth slots} written at the end of the iteration
void launch_update(const BaView& v, float* poses, float* disps, const float* intr, const float* weights,
                   const int64_t* ii, const int64_t* jj, const double* x, float* dx_out, float* dz_out,
                   bool motion_only, hipStream_t s, int* status_mirror = nullptr);
// The Cholesky solve of a CholSystem (chol.hip), damped: diag += ep + lm * diag.  launch_chol_solve = the preset
// (unless done), launch_chol_factor, launch_chol_backsolve; launch_chol_factor returns whether the single-launch
// kernel (chol_factor_persistent_kernel<false>: step-major scheduler) ran, and launch_chol_backsolve needs that answer.
void launch_chol_preset(const CholSystem& c, hipStream_t s);
bool launch_chol_factor(const CholSystem& c, double lm, double ep, hipStream_t s);
void launch_chol_backsolve(const CholSystem& c, bool factor_single, hipStream_t s);
void launch_chol_solve(const CholSystem& c, double lm, double ep, hipStream_t s, bool preset_done);

// Overlap mode (multi-GPU): block columns [J0, J1) of the all-reduced packed system -> pitched matrix, damped; then
// ready[J0..J1) = epoch for the factorisation that is already running.  launch_chol_factor_overlap starts that
// single-launch factorisation (chol_factor_persistent_kernel<true>: per-tile scheduler; false: not available for this
// system, nothing was launched); launch_chol_backsolve(c, true, s) follows it.
void launch_unpack_cols(const BaView& v, int J0, int J1, double lm, double ep, int epoch, hipStream_t s);
bool launch_chol_factor_overlap(const CholSystem& c, const int* ready, int epoch, hipStream_t s);
// whether launch_chol_factor_overlap can take a system of n unknowns on the current device: from n, the device and the
// process-wide switches alone, so that every rank of a group answers alike
bool chol_overlap_available(int n);

}  // namespace droid
