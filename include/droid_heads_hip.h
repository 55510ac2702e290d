/*
 * droid_heads_hip.h -- C ABI of the output heads of the update operator: the last layer of `delta` and of `weight`
 * (droid_slam/droid_net.py:95-106, :130-134: a Conv2d(128, 2, 3, padding=1), the gradient clip -- the identity in
 * forward --, for `weight` a Sigmoid, then `.view(...).permute(0,1,3,4,2)[..., :2].contiguous()`) and of `GraphAgg.eta`
 * (:51-54, :72-75: a Conv2d(128, 1, 3, padding=1), the clip, a Softplus and `.01 *`), under autocast, in ONE launch per
 * call that writes the layout droid_ba_inputs reads.  The conventions, the library (libdroid_backends_hip.so),
 * DROID_ABI_VERSION and the status codes are those of droid_backends_hip.h and droid_update_hip.h.  Binding table:
 * droid_backends/_lib.py ABI_HEADS (tests/test_update_heads_abi.py holds it against the prototypes here).
 *
 * For head k of a call, x_k [B,128,H,W] half, contiguous:
 *
 *   t[b,n,v,u]     = sum_{c,ky,kx} x_k[b,c,v+ky-1,u+kx-1] * w16_k[n,c,ky,kx]  +  float(b16_k[n])    x = 0 outside the image
 *   out_k[b,v,u,n] = half( act_k(t) )                                          out_k: [B, H, W, n_out_k] half
 *
 * w16 = half(weight), b16 = half(bias), nearest-even from the fp32 parameters (autocast's cast); n_out in {1, 2}.
 * Arithmetic: every product x * w16 is exact in fp32; fp32 accumulation, in an order that is fixed but not specified;
 *   + float(b16[n]) in fp32; the activation is evaluated in fp32 ON THE fp32 SUM, with no intermediate half; then ONE
 *   rounding to half, nearest-even.
 *     DROID_HEAD_IDENTITY       y = t
 *     DROID_HEAD_SIGMOID        y = 1 / (1 + expf(-t)), IEEE division: 0 and 1 at the saturated ends, never a NaN
 *                               for a finite t
 *     DROID_HEAD_SOFTPLUS_CENTI y = 0.01f * (t > 20 ? t : log1pf(expf(t))): torch's Softplus(beta=1, threshold=20)
 *                               followed by `.01 *`
 *   No atomics: the same bits on every run.  The bits of batch element b depend neither on B, nor on its position in
 *   the batch, nor on the other head of the call, nor on what ran before.  A NaN or an inf in x reaches exactly the
 *   outputs whose 3 x 3 window (same head, same b) contains it; every other output keeps its bits.  Outputs do not
 *   alias inputs.  All offsets are 64-bit.
 *
 * heads in {1, 2}: all heads of a call share B, H, W and run in one launch (delta + weight: heads = 2, B = E; eta:
 *   heads = 1, B = G).  x, packed, out are arrays of `heads` pointers, n_out and act arrays of `heads` ints.
 *
 * packed_k: the parameters of head k, packed once per network, droid_head_packed_bytes(n_out_k) bytes of FLOAT32,
 *   16-byte aligned.  With n = n_out_k:
 *     element ((c * 3 + ky) * 3 + kx) * n + j,  c < 128, ky < 3, kx < 3, j < n   is float(w16[j][c][ky][kx])
 *     element 1152 * n + j,                     j < n                             is float(b16[j])
 *     elements 1153 * n .. 1153 * n + pad - 1                                     are ZERO, pad = 2 for n = 2 and 3 for
 *                                                                                 n = 1 (the size is a multiple of 16)
 *   so droid_head_packed_bytes(2) = 9232 and droid_head_packed_bytes(1) = 4624; any other n_out answers 0.  The values
 *   are halves widened to fp32, which is exact: the kernel reads them on the scalar path and never converts a weight.
 *   The kernel does not read the padding entries.  It writes every LDS byte its operands read, whatever the LDS held
 *   before.
 *
 * Refusals, DROID_E_ARG with a message that names update_heads and the argument, before any HIP call, sizes before
 * pointers, in this order: heads not in {1, 2} ; B outside [0, 65535] ; H or W < 1 or H * W > 2^30 ; in_channels != 128 ;
 * an n_out not in {1, 2} ; an act outside the enum (n_out and act are read only when the arrays are given; a null array
 * is a null pointer, below) ; then, for B > 0: a null among the five arrays or their first `heads` entries ; a packed_k
 * that is not 16-byte aligned.  B == 0 launches nothing and returns DROID_OK, after the size checks.  There is no
 * fallback: the stock layers stay available.
 */
#ifndef DROID_HEADS_HIP_H
#define DROID_HEADS_HIP_H

#include "droid_update_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { DROID_HEAD_IDENTITY = 0, DROID_HEAD_SIGMOID = 1, DROID_HEAD_SOFTPLUS_CENTI = 2 };

size_t droid_head_packed_bytes(int n_out);
int droid_update_heads(const void* const* x, const void* const* packed, void* const* out, const int* n_out,
                       const int* act, int heads, int B, int H, int W, int in_channels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DROID_HEADS_HIP_H */
