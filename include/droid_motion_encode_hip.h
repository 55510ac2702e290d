/*
 * droid_motion_encode_hip.h -- C ABI of the fused motion encoder: the prologue of an update step on the motion branch,
 * reproject + motion features (droid_slam/factor_graph.py:203-205) followed by `flow_encoder[0:2]` of the update module,
 * a Conv2d(4, 128, 7, padding=3) and a ReLU under autocast (droid_slam/droid_net.py:89-93, :126), in ONE launch that
 * never writes the [E,4,H,W] motion planes.  The conventions, the library (libdroid_backends_hip.so), DROID_ABI_VERSION,
 * the status codes and DROID_CORR_ENCODE_PACKED_BYTES are those of droid_backends_hip.h and droid_update_hip.h.  Binding
 * table: droid_backends/_lib.py ABI_MOTION_ENCODE (tests/test_motion_encode_abi.py holds it against the prototypes here).
 *
 *   y[e,n,v,u] = relu( half( sum_{c,ky,kx} a[e,c,v+ky-3,u+kx-3] * w16[n,c,ky,kx]  +  float(b16[n]) ) )
 *                                                                                        y: [E, 128, H, W] half
 *
 * The operand a.  a[e,c,.,.] = half(m[e,c,.,.]), nearest-even (autocast's cast in front of the convolution), and a = 0
 *   outside the image (padding=3).
 *   motn_in == NULL: m is what droid_reproject_motion writes as motn for the same poses, disps, intrinsics, intr_stride,
 *     ii, jj, target, nbuf, H, W, bit for bit -- the kernel calls that operator's own device function: back-projection
 *     with the source frame's intrinsics and projection with the target frame's (intr_stride 4: intrinsics [nbuf,4];
 *     0: one [4] for all frames), the fixed stereo baseline for ii == jj, a depth below 0.5 * MIN_DEPTH replaced by 1,
 *     and the clamp to +-64 as fminf(fmaxf(.)), so m is always finite and within +-64.  An edge whose ii or jj lies
 *     outside [0, nbuf) (compared as the int64 it is) has m = 0: its y is relu(b16[n]) everywhere and its coords / valid
 *     are zeros.  coords [E,H,W,2] and valid [E,H,W] receive the bits droid_reproject_motion writes there.
 *   motn_in != NULL: m = motn_in, [E,4,H,W] fp32 (values beyond the range of half overflow to inf in the cast).  poses,
 *     disps, intrinsics, ii, jj, target, coords and valid are not looked at and may be NULL; intr_stride and nbuf are
 *     still checked.  The same kernel with another patch loader.
 * w16 = half(weight), b16 = half(bias), nearest-even from the fp32 parameters of flow_encoder[0] ([128,4,7,7], [128]).
 * Arithmetic: every product a * w16 is exact in fp32; fp32 accumulation (v_mfma_f32_16x16x32_f16), in an order that is
 *   fixed but not specified; then + float(b16[n]) in fp32, ONE rounding to half, then max(., 0) (+0 for every value not
 *   above zero; a NaN stays a NaN).  No atomics: the same bits on every run, and the bits of an edge depend neither on E,
 *   nor on its position in the batch, nor on what ran before.
 *
 * packed: the parameters, packed once per network, in the layout of DROID_CORR_ENCODE_PACKED_BYTES (droid_update_hip.h)
 *   unchanged, with "level" read as motion channel: halves [4 channels][2 K steps][8 channel tiles][64 lanes][8], then
 *   b16 [128]; 16-byte aligned.  Element (c, s, nt, lane, j) is w16[16 nt + (lane & 15)][c][kk / 7][kk % 7] with
 *   kk = 32 s + 8 (lane >> 4) + j, and ZERO where kk >= 49: weight.reshape(128, 196) has k = 49 c + 7 ky + kx, so one
 *   packer serves both encoders.  The kernel writes every LDS byte its matrix operands read, the padding columns
 *   49..63 included, whatever the LDS held before.
 *
 * Refusals, DROID_E_ARG with a message that names motion_encode and the argument, before any HIP call, sizes before
 * pointers: E outside [0, 65535] ; H or W < 1 or H * W > 2^30 ; nbuf < 1 ; out_channels != 128 ; intr_stride not in
 * {0, 4} ; then, for E > 0: a null packed or out, a packed that is not 16-byte aligned ; without motn_in, any null among
 * poses, disps, intrinsics, ii, jj, target, coords, valid.  E == 0 launches nothing and returns DROID_OK.  There is no
 * fallback: the unfused sequence (droid_reproject_motion, then the framework's convolution) stays available.
 * droid_motion_encode_packed_bytes is host arithmetic: DROID_CORR_ENCODE_PACKED_BYTES.
 */
#ifndef DROID_MOTION_ENCODE_HIP_H
#define DROID_MOTION_ENCODE_HIP_H

#include "droid_update_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t droid_motion_encode_packed_bytes(void);
int droid_motion_encode(const float* poses, const float* disps, const float* intrinsics, int intr_stride,
                        const int64_t* ii, const int64_t* jj, const float* target, const float* motn_in,
                        const void* packed, float* coords, float* valid, void* out, int E, int nbuf, int H, int W,
                        int out_channels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DROID_MOTION_ENCODE_HIP_H */
