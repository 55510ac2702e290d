/*
 * droid_backends_hip.h -- C ABI of the MI355X (gfx950) implementation of DROID-SLAM's
 * correlation-lookup + dense bundle-adjustment hot path.
 *
 * This is the drop-in boundary: one entry point per operator the reference exports from its
 * `droid_backends` pybind module (/root/reference/src/droid.cpp:237-250).  Signatures carry only
 * raw DEVICE pointers, sizes and a HIP stream (passed as void*, a hipStream_t); no torch types.
 * Every function enqueues on `stream` and returns without synchronising unless stated.
 *
 * Return value: 0 on success, a negative DROID_E_* code on a contract violation detected on the
 * host.  Violations only a kernel can see (index out of range, eta rows != depth slots) are
 * written to the status word in the BA workspace (see droid_ba_status).
 *
 * Tensor layouts are exactly the reference's (row-major, contiguous):
 *   poses  [nbuf,7]  f32  (tx ty tz qx qy qz qw), world->camera     depth_video.py:33
 *   disps  [nbuf,H,W] f32 ; disps_sens [nbuf,H,W] f32 ; intrinsics [4] f32 (fx fy cx cy)
 *   targets, weights [E,2,H,W] f32 ; eta [M,H,W] f32 ; ii, jj [E] int64
 *
 * A second header, droid_update_hip.h, declares the operators between the update network and `ba` (the BA inputs of a
 * factor-graph update) with the same conventions; the same library exports them.
 */
#ifndef DROID_BACKENDS_HIP_H
#define DROID_BACKENDS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DROID_ABI_VERSION 1

#define DROID_OK 0
#define DROID_E_ARG (-1)       /* bad size / null pointer / unsupported dtype            */
#define DROID_E_WORKSPACE (-2) /* workspace too small                                    */
#define DROID_E_HIP (-3)       /* a HIP runtime call failed (see droid_last_error)       */

/* element types of the correlation operators (AT_DISPATCH_FLOATING_TYPES_AND_HALF,
 * correlation_kernels.cu:145, altcorr_kernel.cu:308) */
#define DROID_F16 0
#define DROID_F32 1
#define DROID_F64 2

int droid_abi_version(void);
const char *droid_last_error(void); /* thread-local message of the last failing call */

/* ------------------------------------------------------------------ correlation lookups */

/* Limits of the four volume operators below (droid_corr_index_forward / _backward, droid_corr_pyramid_forward and its
 * _slots form): H1 * W1 <= 2^27 and H2 * W2 <= 2^27 (a query pixel index and the byte count of one plane are 32-bit),
 * else DROID_E_ARG with a message that names the operator and "map size"; B <= 65535.  Offsets into the volumes and the
 * outputs are 64-bit: B (or cap) * H1 * W1 * H2 * W2 may be any size the device holds (tests/test_gpu_large_offsets.py
 * runs them beyond 2^32 elements and 8 GiB). */

/* corr_index_forward (droid.cpp:170-178 -> correlation_kernels.cu:126-155).
 * volume [B,H1,W1,H2,W2] dtype ; coords [B,2,H1,W1] f32 ; corr [B,2r+1,2r+1,H1,W1] dtype
 * (written completely; the caller need not zero it). */
int droid_corr_index_forward(const void *volume, const float *coords, void *corr, int B, int H1,
                             int W1, int H2, int W2, int radius, int dtype, void *stream);

/* CorrBlock.__call__ over all pyramid levels (droid_slam/modules/corr.py:40-50): level l looks
 * up volumes[l] ([B,H1,W1,H1>>l,W1>>l], dtype) at coords * 2^-l (exact) and writes channels
 * [l (2r+1)^2, (l+1) (2r+1)^2) of corr [B, levels (2r+1)^2, H1, W1] = torch.cat(out_pyramid, dim=2) of the
 * reference (with its leading dimension of 1 dropped), without the cat and the per-level coordinate tensors.
 * volumes: HOST array of `levels` device pointers; coords [B,2,H1,W1] f32 at level-0 scale.  Values are
 * bit-identical to droid_corr_index_forward per level.  radius 3 or 4.  Not one of the reference's nine operators. */
int droid_corr_pyramid_forward(const void *const *volumes, const float *coords, void *corr, int B, int H1,
                               int W1, int radius, int levels, int dtype, void *stream);

/* CorrBlock.__init__ for a list of edges in one launch (droid_slam/modules/corr.py:24-38, 63-71, as factor_graph.py:
 * 112-117 calls it), from the feature buffer as DepthVideo holds it.  Not one of the reference's nine operators.
 * fmaps [nbuf, ncam, C, H, W] dtype T (f16 or f32), channels first, ncam 1 or 2 ; ii, jj [E] int64.
 * Edge e: A = fmaps[ii[e], 0], B = fmaps[jj[e], c], c = 1 when ncam == 2 and ii[e] == jj[e], else 0 (with ncam == 1
 * the reference raises on ii == jj; here camera 0 is used).  a = T(A / 4), b = T(B / 4), rounded to T first;
 *   level 0:   vol[e, p, q] = T(sum_c a[c, p] * b[c, q]), p, q flat pixel indices, products and sum in fp32;
 *   level l+1: T(fp32(((v00 + v01) + v10) + v11) * 0.25f) of the ROUNDED level l over the (H2, W2) plane, size
 *              (H >> (l+1), W >> (l+1)) -- avg_pool2d(., 2, stride=2) on dtype T bit for bit, odd sizes floor.
 * levels_out: HOST array of `levels` (1..4) device pointers, level l = [cap, H, W, H>>l, W>>l] of T
 * (CorrBlock.corr_pyramid[l], what droid_corr_pyramid_forward takes).  Edge e is written to slot slot0 + e, completely;
 * no other slot is touched (slot0 + E <= cap).  An edge with ii or jj outside [0, nbuf) yields zeros.  No atomics: the
 * same bits on every run, and an edge's bits do not depend on E or on its slot.
 * C % 32 == 0, C <= 256 ; H, W >= 8, W % 8 == 0, H * W % 16 == 0 ; anything else returns DROID_E_ARG with a message
 * (there is no fallback).  All argument checks are host-side and precede any HIP call; E == 0 launches nothing. */
int droid_corr_volume_pyramid(const void *fmaps, const int64_t *ii, const int64_t *jj, void *const *levels_out,
                              int E, int nbuf, int ncam, int C, int H, int W, int levels, int64_t slot0,
                              int64_t cap, int dtype, void *stream);

/* The two operators above on capacity buffers whose slots are handed out in any order, so that dropping edges
 * (FactorGraph.rm_factors, `self.corr = self.corr[~mask]`) edits a list of integers and moves no pyramid bytes.
 * volumes[l] / levels_out[l]: HOST arrays of device pointers, level l = [cap, H1, W1, H1>>l, W1>>l] of dtype.
 * slots: DEVICE array, [B] / [E] int64; the host never reads it, so its values are checked on the device.
 *
 * droid_corr_pyramid_forward_slots: batch entry b looks up the planes of slot slots[b]; coords [B,2,H1,W1] and
 * corr [B, levels (2r+1)^2, H1, W1] stay indexed by b.  Bit-identical to droid_corr_pyramid_forward on the gathered
 * copy volumes[l][slots]; two entries may name one slot.  A slot outside [0, cap) gives zeros for the whole output of
 * that entry (the convention of an edge index outside [0, nbuf) below and in droid_altcorr_pyramid_forward) and reads
 * nothing outside the buffers.  f16 / f32 / f64, radius 3 or 4, levels 1..8, B <= 65535.
 *
 * droid_corr_volume_pyramid_slots: edge e is written to slot slots[e], completely, with the bits
 * droid_corr_volume_pyramid gives it; no other slot is touched.  An edge whose slot is outside [0, cap) is skipped:
 * nothing is written for it.  Two edges of one call with the same slot violate the contract: which edge's bits end up
 * there is unspecified (nothing outside that slot is written).  f16 / f32; shape limits as above.
 *
 * Both: cap < 1, a null slots with B (E) > 0, and every limit of the function above return DROID_E_ARG with a message.
 * All argument checks are host-side and precede any HIP call; B == 0 / E == 0 launches nothing. */
int droid_corr_pyramid_forward_slots(const void *const *volumes, const int64_t *slots, const float *coords,
                                     void *corr, int B, int64_t cap, int H1, int W1, int radius, int levels,
                                     int dtype, void *stream);
int droid_corr_volume_pyramid_slots(const void *fmaps, const int64_t *ii, const int64_t *jj,
                                    void *const *levels_out, const int64_t *slots, int E, int nbuf, int ncam,
                                    int C, int H, int W, int levels, int64_t cap, int dtype, void *stream);

/* corr_index_backward (droid.cpp:180-191 -> correlation_kernels.cu:157-185).
 * corr_grad [B,2r+1,2r+1,H1,W1] dtype ; volume_grad [B,H1,W1,H2,W2] dtype (written completely). */
int droid_corr_index_backward(const float *coords, const void *corr_grad, void *volume_grad, int B,
                              int H1, int W1, int H2, int W2, int radius, int dtype, void *stream);

/* altcorr_forward (droid.cpp:193-203 -> altcorr_kernel.cu:290-319).
 * fmap1 [B,H1,W1,C], fmap2 [B,H2,W2,C] dtype ; coords [B,N,H1,W1,2] f32 ;
 * corr [B,N,(2r+1)^2,H1,W1] dtype, channel = ix*(2r+1)+iy (written completely). */
int droid_altcorr_forward(const void *fmap1, const void *fmap2, const float *coords, void *corr,
                          int B, int N, int H1, int W1, int H2, int W2, int C, int radius,
                          int dtype, void *stream);

/* AltCorrBlock.corr_fn fused over the pyramid levels (droid_slam/modules/corr.py:105-125; SURVEY.md
 * section 8f row 2): for edge e, level l: altcorr_forward(pyramid[0][ii[e]], pyramid[l][jj[e]],
 * coords[e] / 2^l, r), all levels in one launch and without the per-edge feature-map copies
 * (`pyramid[i][:, jj]`) the Python code makes.
 * pyramid: HOST array of `levels` device pointers, level l = [frames, H>>l, W>>l, C] f32 channels
 * last (AltCorrBlock.pyramid[l] with its leading batch dimension of 1 dropped);
 * ii, jj [E] int64 ; coords [E,H,W,2] f32 (one coordinate set) ;
 * corr [E, levels*(2r+1)^2, H, W] f32 = torch.cat of the per-level results (written completely).
 * fp32, C % 16 == 0, C <= 128, r in {3,4}, levels <= 4; anything else returns DROID_E_ARG and the
 * caller keeps using droid_altcorr_forward per level.  An edge index outside [0,frames) gives zeros. */
int droid_altcorr_pyramid_forward(const float *const *pyramid, const int64_t *ii, const int64_t *jj,
                                  const float *coords, float *corr, int E, int frames, int H, int W,
                                  int C, int radius, int levels, void *stream);

/* The same operator for the pyramid the SLAM path actually holds: `AltCorrBlock(self.video.fmaps[None])`
 * (factor_graph.py:260-261) is built from the HALF feature buffer (depth_video.py:44), `/ 4.0` and `avg_pool2d`
 * stay in half (modules/corr.py:97-104), and `corr_fn` widens the gathered per-edge copies with `.float()`
 * (:120) before the fp32 kernel.  This entry point takes that half pyramid as it is -- level l =
 * [frames, H>>l, W>>l, C] f16 channels last -- and returns the fp32 tensor the reference's
 * `altcorr_forward(fmap1.float(), fmap2.float(), ...)` calls return: products of two halves are exact in fp32 and
 * the dot products are accumulated in fp32 on v_mfma_f32_16x16x32_f16, so only the summation order over channels
 * differs (<= 1e-6 of the output scale; half subnormals are not flushed).  No `.float()` copies, half the feature
 * bytes, 16x the matrix rate of the fp32 path.  C % 32 == 0, C <= 128; otherwise as above. */
int droid_altcorr_pyramid_forward_f16(const void *const *pyramid, const int64_t *ii, const int64_t *jj,
                                      const float *coords, float *corr, int E, int frames, int H, int W,
                                      int C, int radius, int levels, void *stream);

/* altcorr_backward (droid.cpp:205-217 -> altcorr_kernel.cu:322-355), fp32 only like the reference.
 * fmap1_grad/fmap2_grad must be zero-filled by the caller (atomic accumulation);
 * coords_grad is not written (the reference returns zeros). */
int droid_altcorr_backward(const float *fmap1, const float *fmap2, const float *coords,
                           const float *corr_grad, float *fmap1_grad, float *fmap2_grad, int B,
                           int N, int H1, int W1, int H2, int W2, int C, int radius, void *stream);

/* ------------------------------------------------------------------ bundle adjustment */

/* Bytes of device scratch one `ba` call needs (host-only arithmetic, no HIP call).
 * M = rows of eta = number of depth slots |unique(ii) U [t0,t1)| (0 when motion_only). */
size_t droid_ba_workspace_bytes(int E, int nbuf, int H, int W, int t0, int t1, int M);

/* ba (droid.cpp:88-117 -> droid_kernels.cu:1314-1434): `iterations` Gauss-Newton steps, poses
 * and disps updated in place.  dx_out [t1-t0,6] f32 and dz_out [M,H*W] f32 receive the last
 * iteration's updates (dz_out may be NULL when motion_only).  Equivalent to
 * droid_ba_prepare + iterations x (droid_ba_build, droid_ba_solve_update). */
int droid_ba(float *poses, float *disps, const float *intrinsics, const float *disps_sens,
             const float *targets, const float *weights, const float *eta, const int64_t *ii,
             const int64_t *jj, int E, int nbuf, int H, int W, int M, int t0, int t1,
             int iterations, float lm, float ep, int motion_only, float *dx_out, float *dz_out,
             void *workspace, size_t workspace_bytes, void *stream);

/* Phase API (what the multi-GPU driver calls; single-GPU `droid_ba` is built from it).
 *
 * own0/own1: the frames whose depth maps this rank owns.  Edges passed to a rank must all have
 * ii in [own0,own1); window frames outside it create no depth slot here.  Single GPU: 0, nbuf.
 * A rank whose range holds no window frame and that has no edge (more ranks than source frames) passes E = 0, M = 0,
 * eta = NULL: its build writes zeros, its solve_update retracts the poses like every other rank's.  M = 0 with edges
 * is refused (DROID_E_ARG), unless motion_only.
 *
 * droid_ba_prepare: once per call -- depth-slot table, CSR of edges by source frame.
 * droid_ba_build:   one linearisation: writes this rank's contribution to the reduced camera
 *                   system into the workspace: S = [ A - E C^-1 E^T ; b^T ] as a dense fp64
 *                   row-major matrix of 6P+1 rows with row pitch ld = roundup16(6P+1), lower
 *                   triangle valid, row 6P = rhs, no damping yet.  droid_ba_system() returns its device address so that the
 *                   caller can all-reduce (sum) it over ranks (RCCL) before the solve.
 * droid_ba_solve_update: damping (diag += ep + lm*diag), Cholesky, solve, depth
 *                   back-substitution for the owned slots (the E rows are recomputed from
 *                   weights / disparities / the not yet retracted poses, never stored), SE3 /
 *                   disparity retraction.
 */
int droid_ba_prepare(const int64_t *ii, const int64_t *jj, int E, int nbuf, int H, int W, int M,
                     int t0, int t1, int own0, int own1, int motion_only, void *workspace,
                     size_t workspace_bytes, void *stream);

int droid_ba_build(const float *poses, const float *disps, const float *intrinsics,
                   const float *disps_sens, const float *targets, const float *weights,
                   const float *eta, const int64_t *ii, const int64_t *jj, int E, int nbuf, int H,
                   int W, int M, int t0, int t1, int motion_only, void *workspace,
                   size_t workspace_bytes, void *stream);

/* Multi-GPU variant of the build phase: the rank's contribution goes to a PACKED copy of the system -- the lower
 * triangle + rhs row by block columns of 64: block column J holds rows 64 J .. 6P (row 6P = rhs) as rows of w_J
 * doubles (w_J = 64, the last one 6P - 64 J), block columns one after the other --
 * which droid_ba_packed_system() exposes as one contiguous fp64 tensor of *n_elements values: all-reduce (sum) it
 * over the ranks as it is (half the bytes of the pitched matrix, no gather / scatter of the triangle), then call
 * droid_ba_unpack_system (one launch: packed -> the pitched matrix the solver factors in place) and
 * droid_ba_solve_update.  Argument meaning as droid_ba_build. */
int droid_ba_build_packed(const float *poses, const float *disps, const float *intrinsics,
                          const float *disps_sens, const float *targets, const float *weights,
                          const float *eta, const int64_t *ii, const int64_t *jj, int E, int nbuf, int H,
                          int W, int M, int t0, int t1, int motion_only, void *workspace,
                          size_t workspace_bytes, void *stream);
double *droid_ba_packed_system(void *workspace, int E, int nbuf, int H, int W, int t0, int t1, int M,
                               size_t *n_elements);
int droid_ba_unpack_system(int E, int nbuf, int H, int W, int M, int t0, int t1, int motion_only,
                           void *workspace, size_t workspace_bytes, void *stream);

/* Overlap of the collective with the solve (multi-GPU, opt-in).  The factorisation consumes
 * block columns left to right and the packed system is block-column major, so a PREFIX of it is all the leading
 * block columns need.  droid_ba_overlap_plan cuts the packed tensor into at most max_chunks contiguous element
 * ranges [packed_offsets[c], packed_offsets[c+1]) of 1, 1, 2, 3, 4, ... block columns.  Per iteration:
 *   main stream : droid_ba_build_packed ... droid_ba_solve_update_overlap(epoch)   -- launched BEFORE the reduction;
 *                 its factorisation waits, tile by tile, for the block columns it is about to read
 *   side stream : (after the build) for c = 0 .. nchunks-1: all-reduce chunk c of the packed tensor in place, then
 *                 droid_ba_unpack_chunk(c, lm, ep, epoch): columns -> pitched matrix with the damping applied, then
 *                 the block columns are published for `epoch`.
 * epoch = 1, 2, ... within one droid_ba_prepare (which resets the published epochs).  The spinning grid leaves
 * DROID_OVERLAP_RESERVE_CUS (default 32) compute units free for the collective's kernels.  Returns DROID_E_ARG
 * when the single-launch solver cannot run this system (then: droid_ba_unpack_system + droid_ba_solve_update).
 * Rehearsed with two ranks on one GPU (gloo) and with eight in-process shards; NOT yet measured over RCCL.
 *
 * Every rank of a group must issue the same collectives, so whether an iteration is cut into chunks may depend only on
 * what the ranks share.  droid_ba_overlap_available answers from the window size, the current device and the
 * process-wide solver switches alone (1: droid_ba_solve_update_overlap takes such a system, 0: it would return
 * DROID_E_ARG); it reads no workspace.  A rank WITHOUT edges cannot spin (droid_ba_solve_update_overlap needs the
 * preset of a build with edges): it all-reduces the same chunks as its peers, then calls droid_ba_unpack_system and
 * droid_ba_solve_update. */
int droid_ba_overlap_available(int t0, int t1);
int droid_ba_overlap_plan(int t0, int t1, int max_chunks, int *nchunks_out, size_t *packed_offsets);
int droid_ba_unpack_chunk(int E, int nbuf, int H, int W, int M, int t0, int t1, int chunk, int max_chunks, float lm,
                          float ep, int epoch, void *workspace, size_t workspace_bytes, void *stream);
int droid_ba_solve_update_overlap(float *poses, float *disps, const float *intrinsics, const float *weights,
                                  const int64_t *ii, const int64_t *jj, int E, int nbuf, int H, int W, int M,
                                  int t0, int t1, int epoch, int motion_only, float *dx_out, float *dz_out,
                                  void *workspace, size_t workspace_bytes, void *stream);

int droid_ba_solve_update(float *poses, float *disps, const float *intrinsics, const float *weights,
                          const int64_t *ii, const int64_t *jj, int E, int nbuf, int H, int W, int M,
                          int t0, int t1, float lm, float ep, int motion_only, float *dx_out,
                          float *dz_out, void *workspace, size_t workspace_bytes, void *stream);

/* Measurement support (bench.py): one Gauss-Newton iteration after droid_ba_prepare with a HIP
 * event between kernel groups on `stream`; synchronises.  stage_ms[8] = {memset+linearise,
 * assemble, fused E-rows + Schur SYRK + rhs, (unused: 0), damp+Cholesky factor, triangular
 * back-solve, state update, total}. */
int droid_ba_profile_iteration(float *poses, float *disps, const float *intrinsics,
                               const float *disps_sens, const float *targets, const float *weights,
                               const float *eta, const int64_t *ii, const int64_t *jj, int E,
                               int nbuf, int H, int W, int M, int t0, int t1, float lm, float ep,
                               int motion_only, void *workspace, size_t workspace_bytes,
                               void *stream, float *stage_ms);

/* Device address / element count of the dense fp64 system inside the workspace. */
double *droid_ba_system(void *workspace, int E, int nbuf, int H, int W, int t0, int t1, int M,
                        size_t *n_elements);

/* Blocking read of the workspace status word: 0 ok; bit0 index out of range; bit1 eta rows !=
 * depth slots; bit2 Cholesky failed in the last solve (not positive definite: dx = 0, like
 * droid_kernels.cu:1207-1210 -- the reference's behaviour, not an error); bit3 the single-launch solver's
 * grid stalled (another spinning grid of a different PROCESS held the CUs; dx = 0; an error: run such
 * deployments with DROID_CHOL_COOPERATIVE=1 or DROID_CHOL_MULTI_LAUNCH=1). */
int droid_ba_status(const void *workspace, void *stream, int *status_out, int *depth_slots_out);

/* Non-blocking error reporting: `mirror` points to 4 ZEROED ints of page-locked host memory that the device can
 * address (hipHostMalloc / torch pin_memory).  Every droid_ba_solve_update on this workspace then ends by
 * writing {status word, depth slots} to words 0 / 1 (system-scope stores by the last kernel of the iteration), and,
 * when the iteration ended with bit0, bit1 or bit3 set, by incrementing word 2 and OR-ing the status into word 3.
 * Words 2 / 3 are STICKY -- only the device writes them, nothing resets them -- so a violation of call k is still
 * there after call k+1 has been enqueued and has reset the workspace's own status word: the host compares word 2
 * with the count it has already reported, whenever it likes, without synchronising the stream.
 * mirror = NULL detaches.  The registration is host-side (keyed by the workspace address).
 *
 * Preconditions of the phase API on one workspace: droid_ba_build and droid_ba_solve_update alternate on ONE
 * stream (build presets the solver scratch that solve_update consumes); concurrent `ba` calls need separate
 * workspaces (droid_backends keeps one per (device, stream)). */
int droid_ba_attach_status_mirror(const void *workspace, int *mirror);

/* Launch hints (optional): `hints` points to 2 ints of page-locked host memory that the device can address (attaching
 * zeroes them; tags are unique in the process, so a late hint of an earlier prepare is never taken for the current one).
 * droid_ba_prepare's kernel then writes {tag of that prepare, number of depth slots of Schur class 3 (more edges than the
 * regular Schur kernels take: block pairs)} there, and droid_ba_build / droid_ba leave the block-pair launch of an
 * iteration out when the hint of the CURRENT prepare has arrived and says "none" (most graphs: 5 us per iteration).
 * The host never waits for the hint: not there yet = launch.  Results do not depend on it.  hints = NULL detaches. */
int droid_ba_attach_launch_hints(const void *workspace, int *hints);

/* The wave-level sum of the linearisation (exposed for tests): one 64-lane wave, lane l holding in[l][0..31], runs the
 * halving butterfly (partners l^32, l^16, l^8, l^4, l^2, l^1); out[l] = the wave total of value
 * bit5(l) + 2 bit4(l) + 4 bit3(l) + 8 bit2(l) + 16 bit1(l), in the bits that addition tree gives.
 * in [64][32] f32, out [64] f32, device pointers. */
int droid_test_wave_reduce32(const float *in, float *out, void *stream);

/* Dense SPD solve used by the BA (exposed for tests): A [n,n] fp64 row-major (lower triangle
 * read, destroyed), b [n] fp64 -> x [n] fp64.  fail_flag (device int) is set to 1 when a pivot
 * is not positive.  scratch (128-byte aligned): >= droid_chol_scratch_doubles(n) doubles (the augmented system
 * with 128-byte rows, the factored diagonal tiles, hand-over slots of the panel tiles, hand-off flags). */
size_t droid_chol_scratch_doubles(int n);
int droid_chol_solve(const double *A, const double *b, double *x, int n, double *scratch,
                     int *fail_flag, void *stream);

/* ------------------------------------------------------------------ geometry operators */

/* frame_distance (droid.cpp:120-136 -> droid_kernels.cu:518-657, :1438-1460): dist [E] f32 */
int droid_frame_distance(const float *poses, const float *disps, const float *intrinsics,
                         const int64_t *ii, const int64_t *jj, int E, int nbuf, int H, int W,
                         float beta, float *dist, void *stream);

/* All ordered pairs of the first n frames in one launch: dist [n,n] f32, dist[i*n + j] = the value
 * droid_frame_distance gives for the edge i -> j.  This is `DepthVideo.distance()` with ii = None
 * (droid_slam/depth_video.py:160-169: meshgrid indices) and the candidate matrix of add_proximity_factors
 * (factor_graph.py:318-326) without index tensors, and with each depth map fetched once per block of 32
 * targets instead of once per pair (SURVEY.md section 8f row 1 "batched all-pairs variant").  Not one of the
 * reference's nine operators.  poses / disps hold at least nbuf >= n frames. */
int droid_frame_distance_matrix(const float *poses, const float *disps, const float *intrinsics, int n,
                                int nbuf, int H, int W, float beta, float *dist, void *stream);

/* projmap (droid.cpp:139-154 -> droid_kernels.cu:427-516, :1463-1488):
 * coords [E,H,W,3] f32 (channel 2 zero), valid [E,H,W,1] f32.  Any E an int holds (launched in slabs of 65535). */
int droid_projmap(const float *poses, const float *disps, const float *intrinsics,
                  const int64_t *ii, const int64_t *jj, int E, int nbuf, int H, int W,
                  float *coords, float *valid, void *stream);

/* reproject + motion features: what `DepthVideo.reproject` and the three lines after
 * it compute for every update-operator call, in one pass and without lietorch --
 *   droid_slam/depth_video.py:150-158 -> geom/projective_ops.py:96-125 (`projective_transform`: source-frame
 *   intrinsics for the back-projection, target-frame intrinsics for the projection, stereo edges ii == jj use the
 *   baseline (-0.1,0,0), depth < 0.1 projects with depth 1, valid = depth > 0.2), factor_graph.py:203-205
 *   (`motn = cat(coords1 - coords0, target - coords1).permute(0,1,4,2,3).clamp(-64, 64)`).
 * intrinsics: [nbuf,4] with intr_stride = 4, or one [4] for all frames with intr_stride = 0.
 * target [E,H,W,2] f32 and motn [E,4,H,W] f32 may both be null (plain reproject).
 * coords [E,H,W,2] f32, valid [E,H,W,1] f32.  Edges with an index outside [0,nbuf) produce zeros.
 * Any E an int holds (launched in slabs of 65535). */
int droid_reproject_motion(const float *poses, const float *disps, const float *intrinsics, int intr_stride,
                           const int64_t *ii, const int64_t *jj, const float *target, int E, int nbuf, int H,
                           int W, float *coords, float *valid, float *motn, void *stream);

/* iproj (droid.cpp:157-166 -> droid_kernels.cu:779-850, :1518-1541): points [nm,H,W,3] f32.
 * Any nm an int holds (launched in slabs of 65535). */
int droid_iproj(const float *poses, const float *disps, const float *intrinsics, int nm, int H,
                int W, float *points, void *stream);

/* depth_filter (droid.cpp:220-234 -> droid_kernels.cu:661-775, :1491-1515):
 * counter [num,H,W] f32 (written completely).  Any num an int holds (launched in slabs of 65535); an index outside
 * [0,nbuf), compared as the int64 it is, gives a zero plane. */
int droid_depth_filter(const float *poses, const float *disps, const float *intrinsics,
                       const int64_t *ix, const float *thresh, int num, int nbuf, int H, int W,
                       float *counter, void *stream);

/* ------------------------------------------------------------------ convex upsampling */

/* `DepthVideo.upsample` (droid_slam/depth_video.py:134-138) with `cvx_upsample` (droid_net.py:21-35) behind it, in one
 * launch: the gather `disps[ix]`, softmax over the 9 taps, the 3x3 unfold, the weighted sum, the pixel shuffle and the
 * scatter `disps_up[ix] = ...`.  Not one of the reference's nine operators.
 * data [nbuf_in, H, W] f32, the disparity buffer as DepthVideo holds it (only read) ; out [nbuf_out, 8H, 8W] f32 ;
 * mask [n, 576, H, W] of mask_dtype (DROID_F16 or DROID_F32), contiguous, channel c = (k*8 + a)*8 + b with k = ky*3 + kx
 * the tap of the 3x3 neighbourhood and (a, b) the sub-pixel row and column (the reference's
 * `view(batch, 1, 9, 8, 8, ht, wd)`) ; ix [n] int64 on the DEVICE, or NULL for the identity.
 * Entry e uses frame f = ix[e] (e when ix is NULL): it reads data[f] and mask[e] and writes out[f] completely,
 *   out[f, 8y+a, 8x+b] = sum_k w_k * P(y + ky - 1, x + kx - 1),   w = softmax_k(mask[e, (k*8+a)*8+b, y, x]),
 * P = data[f] with zero outside the image (F.unfold(., [3,3], padding=1)).  No other frame of out is touched.
 * Arithmetic, all in fp32: half logits widened exactly, the maximum subtracted first (logits of +-65504 cannot
 * overflow), expf, the sum in ascending k, one division per weight, the products accumulated in ascending k (the first
 * a multiplication, the other eight fused multiply-adds); the weights are never rounded to half, unlike
 * `torch.softmax` of a half mask.  Every output pixel is within 32 * 2^-24 * (max |P| over its neighbourhood) of the
 * fp64 evaluation.  No atomics: the same bits on every run, and the bits of a frame do not depend on n or
 * on the entry's position in the batch.
 * The host never reads ix, so it is checked on the device: an entry whose frame is outside [0, min(nbuf_in, nbuf_out))
 * is skipped -- nothing is read or written for it (the convention of droid_corr_volume_pyramid_slots).  Two entries that
 * name one frame violate the contract: which entry's bits land there is unspecified (nothing outside that frame is
 * written).
 * DROID_E_ARG with a message: mask_dtype not F16 / F32 ; H < 1 or W < 1 ; n < 0 ; nbuf_in < 1 or nbuf_out < 1 ; a null
 * data, mask or out with n > 0 ; 8H * 8W * nbuf_out (or 576 * H * W * n) beyond 2^62 elements, or H * W beyond
 * 2^31 - 65 (the kernel's index types).  All checks are host-side and precede any HIP call; n == 0 launches nothing and
 * returns 0.  Any n an int holds (launched in slabs of 65535); any H, W >= 1: no alignment requirement, no fallback. */
int droid_cvx_upsample(const float *data, const int64_t *ix, const void *mask, float *out, int n, int nbuf_in,
                       int nbuf_out, int H, int W, int mask_dtype, void *stream);

/* ------------------------------------------------------------------ graph aggregation */

/* The source-frame mean of the update operator, `GraphAgg.forward` (droid_slam/droid_net.py:59-75):
 *   _, ix = torch.unique(ii, return_inverse=True) ;  net = scatter_mean(net.view(batch, num, 128, ht, wd), ix, dim=1)
 * (torch_scatter) in two launches on the stream, without atomics and without a host read.  Not one of the reference's
 * nine operators.
 * src [E, plane] and out [M, plane] of `dtype` (DROID_F16 or DROID_F32), contiguous; plane = C*H*W is any value >= 1.
 * No alignment requirement on plane or on the pointers: where src or out is not 16-byte aligned, or the row pitch is
 * not a multiple of 16 bytes, an element-wise path computes the same bits as the 16-byte path.
 * index [E] int64 on the DEVICE.  The host never reads it, so it is checked on the device: an entry outside [0, range)
 * belongs to no group and is ignored.
 * Grouping.
 *  compact = 0 (torch_scatter semantics; needs range == M): row r of out is the mean of the entries with index[e] == r;
 *    a row without entries is +0.0.
 *  compact = 1 (GraphAgg with its torch.unique fused; range = the frame-buffer size): row g is the mean of the entries
 *    whose index is the g-th smallest distinct in-range value.  With fewer distinct values than M the remaining rows
 *    are +0.0; with more, the groups from M onward are not written.
 *  groups_out (device int, may be NULL) receives the number of distinct in-range values (dense mode: the rows that
 *    have an entry), so that a caller can pass a known M without a host synchronisation and check it later.
 * Arithmetic.  For a group with the entries e_0 < e_1 < ... (ascending e) and count n, per element:
 *    acc = float(x[e_0]) ;  acc = acc + float(x[e_k]) for k = 1 .. n-1, in fp32, in that order ;
 *    q = acc / float(n), one correctly rounded fp32 division ;  out = T(q), round to nearest even.
 *  Half inputs are widened exactly, subnormals are kept, nothing is sanitised: NaN and inf propagate by IEEE rules and
 *  a group holding a single -0.0 yields -0.0.  No atomics on out: the same bits on every run.  The bits of a group do
 *  not depend on E, on the other groups or on where its entries sit among foreign ones, only on the order of its own
 *  entries.  Per element |out - exact mean| <= (n + 2) * 2^-24 * (sum |x| / n), plus 2^-11 |mean| + 2^-25 for a half
 *  output.  out is written completely (all M rows); src and index are only read.
 * Limits, DROID_E_ARG with a message that names graph_mean and the argument: E outside 0 .. 65535 ; range < 1 or above
 * DROID_GRAPH_MEAN_MAX_RANGE (the prepare step keeps a count, a presence bitmap and its prefix ranks over [0, range) in
 * LDS) ; M < 1 ; compact not 0 / 1 ; compact = 0 with range != M ; plane < 1, or M * plane or E * plane beyond 2^62 ; a
 * dtype other than F16 / F32 ; a null out, or a null src or index with E > 0 ; a null workspace with E > 0.  A workspace
 * below droid_graph_mean_workspace_bytes(E, range) (host arithmetic: (range + 1 + E) ints; 0 for an E or range refused
 * here): DROID_E_WORKSPACE.  All checks are host-side and precede any HIP call: sizes and dtype, then pointers, then
 * the workspace.  E == 0 zero-fills out, writes 0 to groups_out, needs no workspace and returns 0.  Concurrent calls
 * need separate workspaces.  The prepare step is one workgroup: up to 8192 entries it sorts the lists in LDS (a few
 * microseconds); beyond, one thread per frame walks the index, sized for what a factor graph can hold and no more
 * (milliseconds at E = 65535 with 16384 frames). */
#define DROID_GRAPH_MEAN_MAX_RANGE 16384
size_t droid_graph_mean_workspace_bytes(int E, int range);
int droid_graph_mean(const void *src, const int64_t *index, void *out, int E, int64_t plane, int M, int range,
                     int compact, int dtype, int *groups_out, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ factor-graph edge selection */

/* The edge list `FactorGraph.add_proximity_factors` (droid_slam/factor_graph.py:315-379) hands to `add_factors`,
 * and the duplicate filter `add_factors` starts with (:44-55), selected on the stream from the frame-distance matrix
 * and the edges the graph holds: no host round trip, 4 stream operations whatever t is and however many edges are
 * accepted.  Not one of the reference's nine operators (the reference does this in a host loop with one blocking
 * read per candidate).
 *
 * Rows of the candidate rectangle are frames [t0,t), columns frames [t1,t); t1 <= t0 (else DROID_E_ARG).
 *  1. d[i,j] = 0.5f * (dist[i*ld+j] + dist[j*ld+i]) in fp32 when `bidirectional`, else dist[i*ld+j].  `dist` is the
 *     directed matrix droid_frame_distance_matrix writes (ld >= t floats per row); it is only read.
 *  2. d = inf where i - rad < j, and where d > 100.
 *  3. Every suppressing edge (i,j) -- the caller passes active + bad + inactive edges -- puts d = inf on the cells
 *     (i+di, j+dj) with |di| + |dj| <= max(min(|i-j| - 2, nms), 0) that lie in the rectangle.  Duplicates and edges
 *     anywhere outside the rectangle are fine.
 *  4. Forced edges, in this order: for i in [t0,t): (i,i) when `stereo`; then for j in [max(i-rad-1,0), i): (i,j),
 *     (j,i).  Their cells become inf.
 *  5. The cells in ascending d, ties by ascending flat index (i-t0)*(t-t1) + (j-t1) (the reference's argsort leaves
 *     ties open): skip the cell when its d, as modified so far, is > thresh; STOP when the list already holds more
 *     than max_factors edges; else append (i,j), (j,i) and put the diamond of step 3 around (i,j) to inf.
 *     max_factors = -1 (the FactorGraph default) therefore yields the forced edges only.
 *  6. When n_known > 0: every edge that is in the known list (active + inactive) is dropped, the order kept.
 * edges_out [cap,2] int64 receives the edges, *count_out (device int) their number.  cap must be at least the most
 * steps 4-5 can produce: max(forced, min(max_factors + 2, forced + 2 * cells)) with forced = the count of step 4,
 * cells = (t-t0)*(t-t1).  t <= t0 gives an empty list.
 *
 * Where this differs from the reference's text:
 *  - The reference addresses d by flat index, so in step 4 a column j < t1 lands in another row (or raises
 *    IndexError).  Here a cell outside the rectangle is ignored.  For t1 < t0 and for t1 = t0 = 0 -- every call the
 *    reference makes -- the cell it hits is at inf already and the lists are identical (swept in
 *    tests/test_proximity_ref.py); t1 = t0 > 0 is legal here but outside that claim.
 *  - A cell at inf or NaN is never selected, also not with thresh = inf (`inf > inf` is false in the reference).
 *  - Limits: the suppression bitmap of the rectangle lives in LDS, so cells <= 1048576 (1024 x 1024), and
 *    nms <= 1024; beyond either: DROID_E_ARG.  More than 16384 cells with d <= thresh take a slower sort (LDS sorts
 *    of 16384 + merges by one workgroup); results are the same.
 * Workspace: droid_proximity_workspace_bytes (host arithmetic; 0 for sizes droid_proximity_edges rejects).
 * Concurrent calls need separate workspaces. */
size_t droid_proximity_workspace_bytes(int t, int t0, int t1, int n_known, int cap);
int droid_proximity_edges(const float *dist, int ld, int bidirectional, int t, int t0, int t1, int rad, int nms,
                          float thresh, int max_factors, int stereo, const int64_t *sup_ii, const int64_t *sup_jj,
                          int n_sup, const int64_t *known_ii, const int64_t *known_jj, int n_known,
                          int64_t *edges_out, int cap, int *count_out, void *workspace, size_t workspace_bytes,
                          void *stream);

/* ------------------------------------------------------------------ pose algebra */

/* The SE3 group operations the inference path takes from lietorch -- `PoseTrajectoryFiller.__fill`
 * (droid_slam/trajectory_filler.py:43-58), the visualiser's `SE3(poses).inv().matrix()`, `Droid.terminate`'s final
 * `.inv()`, the multi-session `T.inv() * poses` -- on [n,7] pose records.  Not among the reference's nine operators.
 * None of them acts on points (reproject / iproj own the point actions), none has a gradient.
 * Records are tx ty tz qx qy qz qw, tangents tau_x tau_y tau_z phi_x phi_y phi_z.  Quaternions are used as they are and
 * never renormalised: the rotation of a record is R = I + 2 w [v]x + 2 [v]x^2 whatever its norm.
 * Arithmetic: every value is evaluated in fp64 from the float32 inputs and rounded to float32 once.  Per component
 *   |out - exact| <= 2^-23 |exact| + 2^-36 S,  S = 1 + the largest |translation component| among inputs and result
 * ("pose algebra").  Parity with lietorch itself is unpinned: it cannot be built for this device, so the
 * yardstick is the fp64 restatement of the formulas below (tests/se3_ref.py), not lietorch's own series thresholds.
 *  INV     q' = conj(q), t' = -(q' (*) t)                     ((*): the rotation above)
 *  MATRIX  row-major 4x4, R entry by entry, t in the fourth column, last row 0 0 0 1
 *  EXP     q = (sin(theta/2)/theta phi, cos(theta/2)), t = V tau,
 *          V = I + (1 - cos theta)/theta^2 [phi]x + (theta - sin theta)/theta^3 [phi]x^2; continuous through theta = 0
 *  LOG     phi = 2 atan(n/w)/n v with n = |v|: the rotation vector of least norm, |phi| <= pi; 2/w - (2/3) n^2/w^3 as
 *          n -> 0; +pi v/n when w == 0; log(c q) = log(q) for every c != 0, negative c included (at exactly w == 0
 *          the least-norm vector is not unique, and the + follows the sign of v: -q gives -phi, the same rotation).
 *          tau = V^-1 t, V^-1 = I - 1/2 [phi]x + c [phi]x^2, c = (1 - theta cos(theta/2) / (2 sin(theta/2))) / theta^2.
 *  mul     out[k] = a[k] * b[k]: q = qa qb (Hamilton product), t = ta + qa (*) tb.  stride_a, stride_b are 7, or 0 to
 *          broadcast one record.
 * Each thread reads its records before it writes: out == in is allowed for INV, out == a or out == b for mul where that
 * side's stride is 7.  Any other overlap of out with an input is refused.
 * Refused with DROID_E_ARG and a message naming the function and the argument, before any HIP call: op outside 0 .. 3;
 * n < 0; n * 16 beyond 2^62; a stride other than 0 or 7; a null pointer with n > 0; an overlap as above.  n == 0 launches
 * nothing and returns 0. */
#define DROID_SE3_INV 0     /* in [n,7] -> out [n,7]  */
#define DROID_SE3_LOG 1     /* in [n,7] -> out [n,6]  (tau, phi) */
#define DROID_SE3_EXP 2     /* in [n,6] -> out [n,7]  */
#define DROID_SE3_MATRIX 3  /* in [n,7] -> out [n,16] row-major 4x4, last row 0 0 0 1 */
int droid_se3_unary(const float *in, float *out, int64_t n, int op, void *stream);
int droid_se3_mul(const float *a, int stride_a, const float *b, int stride_b, float *out, int64_t n, void *stream);

/* The linear pose interpolation of `PoseTrajectoryFiller.__fill` (trajectory_filler.py:44-58) in one launch, without
 * the reference's one blocking read per query.  poses [>= N,7], tstamp [>= N], query [M] float32 on the device (the
 * reference compares a Python number with a float32 tensor, so a float32 query reproduces it).  For the query t:
 *   k0 = max(#{k < N : tstamp[k] <= t} - 1, 0)      a count, as in the reference: nothing assumes sorted stamps
 *   k1 = k0 + 1 if k0 < N - 1 else k0
 *   dt = tstamp[k1] - tstamp[k0] + 1e-3
 *   out = exp( log(P[k1] P[k0]^-1) / dt * (t - tstamp[k0]) ) P[k0]
 * all in fp64 (the two stamp differences included), rounded once; the bound above holds with S multiplied by
 * 1 + |t - tstamp[k0]| / dt.  out [M,7]; k0_out, k1_out [M] int64 (either may be NULL) receive the brackets: the `ii`
 * of the edges the filler adds next.  Nothing outside [0, N) is read.
 * Where this differs from the reference: for t before every stamp the reference computes k0 = -1, which wraps to the
 * last keyframe and then goes into `ba` as a frame index.  Here k0 clamps to 0 and the pose is extrapolated backwards
 * from the first bracket.
 * After the last stamp k1 == k0: the relative pose is the exact identity and out = P[k0].  A NaN stamp is never
 * counted.  A NaN query gives k0 = 0 and NaN poses.
 * Refused with DROID_E_ARG before any HIP call: N < 1; M < 0; a null poses / tstamp / query / out with M > 0; out, k0_out
 * or k1_out overlapping an input.  M == 0 launches nothing and returns 0. */
int droid_pose_interpolate(const float *poses, const float *tstamp, int N, const float *query, int M,
                           float *out /*[M,7]*/, int64_t *k0_out /*[M]*/, int64_t *k1_out /*[M]*/, void *stream);

/* ------------------------------------------------------------------ point cloud */

/* The filtered, coloured point cloud of selected keyframes -- the body of the reference fork's viewers and map tools
 * (visualization.py:100-142: index_select, SE3(poses).inv(), iproj, depth_filter, the count / disparity mask, the
 * per-frame boolean indexing on the host) -- selection, filtering, colouring and ordered compaction on the stream, with
 * nothing per pixel on the host.  Not one of the reference's nine operators.
 *
 * Inputs, all on one device, all contiguous, only read:
 *   poses [nbuf,7] float32, world-to-camera, as stored ;  disps [nbuf,H,W] float32 ;  intrinsics [4] float32 ;
 *   index [n] int64 (the host never reads it) ;  thresh [n] float32, one per selection ;
 *   images [nbuf,3,8H,8W] uint8, stored BGR as in `video.images`, or NULL (then colors is NULL too) ;
 *   min_count (the reference uses 2) ;  disp_ratio (the reference uses 0.5).
 * Per selection b with i = index[b].  i outside [0,nbuf), tested as an int64 before any narrowing: the selection yields
 * no point and an all-zero matrix.  Otherwise:
 *  1. Pose inverse.  G = inv(poses[i]) by the pose algebra's contract above: fp64 from the float32 record, the
 *     quaternion as it is.  matrices[b] = matrix(G) rounded once to float32: the value droid_se3_unary gives for INV
 *     followed by MATRIX up to the rounding of the intermediate record.
 *  2. Count.  count[k] = droid_depth_filter's count of frame i against its six temporal neighbours inside [0,nbuf),
 *     with the poses as stored and thresh[b]: the same device code, hence the same bits.
 *  3. Mean.  mean = sum(disps[i]) / (H W), accumulated in fp64; the order of the sum is free.
 *  4. Keep rule.  Pixel k is kept iff count[k] >= min_count and (double)disps[i][k] > disp_ratio * mean.
 *  5. Point.  G (X0 / d), X0 = ((u - cx) / fx, (v - cy) / fy, 1), d = disps[i][k], evaluated in fp64 from the float32
 *     inputs and rounded once: droid_iproj with the inverted pose, without the float32 rounding of that pose.  Per
 *     component |out - exact| <= 2^-23 |exact| + 2^-40 S, S = 8 ((|X0x| + |X0y| + 1) / |d| + |t|_1).
 *  6. Colour (images given).  float(images[i, c, 8v+3, 8u+3]) / 255.0f for c = 2, 1, 0, one IEEE float32 division.
 * Outputs.  Points come in the order of index, row-major within a frame: exactly the concatenation over b of
 * points[b].reshape(-1,3)[mask[b]].  A frame selected twice is emitted twice.
 *   points [P,3] float32 ;  colors [P,3] float32 ;  src [P] int32, the pixel index v W + u of each point ;
 *   offsets [n+1] int32: offsets[0] = 0, selection b owns rows offsets[b] : offsets[b+1], P = offsets[n] ;
 *   matrices [n,4,4] float32, row-major.
 * points, colors and src are capacity buffers of n H W rows; rows at and beyond offsets[n] are NOT written.
 * Three launches on the stream (decisions per 256-pixel tile, one-workgroup scan of the tile counts, emission); beyond
 * 65536 tiles the first and the third go out in slabs of that many.  No atomics, no workgroup waits for another: the
 * same bits on every run.  Every tile's frame mean re-reads the frame (H W floats, from L2).
 * Workspace: droid_point_cloud_workspace_bytes(n, H, W) bytes (host arithmetic: 36 bytes per tile; 0 for sizes refused
 * here), 8-byte aligned.  Every word the call reads it has written itself: nothing depends on what the workspace held.
 * Concurrent calls need separate workspaces.
 * Refused with DROID_E_ARG and a message naming point_cloud and the argument, before any HIP call, sizes before
 * pointers: n < 0 ; H or W < 1 ; n H W >= 2^31 ; nbuf < 1 ; then a null poses / disps / intrinsics / index / thresh /
 * points / src / offsets / matrices ; images without colors or colors without images ; a null, too small or misaligned
 * workspace ; an output (the workspace included) that shares a byte with an input or with another output.  Any
 * H, W >= 1 is accepted: a frame with one row or one column keeps nothing (no projection has its four corners inside).
 * n == 0 launches nothing, touches no pointer and returns 0. */
size_t droid_point_cloud_workspace_bytes(int n, int H, int W);
int droid_point_cloud(const float *poses, const float *disps, const float *intrinsics, const int64_t *index,
                      const float *thresh, const uint8_t *images, int n, int nbuf, int H, int W, int min_count,
                      double disp_ratio, float *points, float *colors, int *src, int *offsets, float *matrices,
                      void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DROID_BACKENDS_HIP_H */
