/*
 * droid_test_hooks_hip.h -- entry points of libdroid_backends_hip.so that exist for its tests only.  A third header next
 * to droid_backends_hip.h with the same conventions (raw DEVICE pointers, sizes, a HIP stream; 0 or a negative DROID_E_*
 * code with a message in droid_last_error; enqueue and return).  Not part of the drop-in boundary: the main header (whose
 * 48 prototypes tests/test_abi.py pins) and DROID_ABI_VERSION do not change when a hook is added here.
 * droid_backends/_lib.py binds it as ABI_TEST, where the loaded library exports it.
 */
#ifndef DROID_TEST_HOOKS_HIP_H
#define DROID_TEST_HOOKS_HIP_H

#include "droid_backends_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The linearisation of droid_ba_build alone (its first stage: the ba_lin_kernel launch, the edge-range sum where the
 * slots' edges are split, and the clearing of the reduced system), on a workspace that droid_ba_prepare has run on.
 * Arguments as droid_ba_build up to motion_only.
 *   ragged != 0: the kernel body with per-lane pixel guards also where H*W is a multiple of the 512-pixel chunk and
 *   the product runs the guard-free body whose roundings are pinned in source.  The two must leave the same bits.
 * Afterwards what the stage left in the workspace is copied (device to device, on `stream`) to the buffers that are not
 * NULL, and words_out[0..5] (host memory, six words, may be NULL) receive their lengths in floats [0..3], whether the
 * graph keeps E rows [4] and the number of edge ranges per (slot, chunk) [5] -- the host's choice of kernel instantiation;
 * with all four buffers NULL the call is a size query and launches nothing:
 *   hpart_out  per-(edge, chunk, wave) partial Hjj + vj   [E][chunks][4][32]
 *   q_out      1 / C                                       [M][H*W]      (0 words when motion_only)
 *   w_out      w                                           [M][H*W]
 *   ebuf_out   unscaled E rows of dense graphs             6 (M + E) H*W, 0 words for graphs that keep none */
int droid_test_ba_lin(const float *poses, const float *disps, const float *intrinsics, const float *disps_sens,
                      const float *targets, const float *weights, const float *eta, const int64_t *ii,
                      const int64_t *jj, int E, int nbuf, int H, int W, int M, int t0, int t1, int motion_only,
                      int ragged, void *workspace, size_t workspace_bytes, float *hpart_out, float *q_out,
                      float *w_out, float *ebuf_out, size_t *words_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DROID_TEST_HOOKS_HIP_H */
