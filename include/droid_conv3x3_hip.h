/*
 * droid_conv3x3_hip.h -- C ABI of the 3 x 3 convolution of the update operator: a Conv2d(C_in, C_out, 3, padding=1)
 * under autocast with an optional ReLU, on half [B,C_in,H,W] planes (droid_slam/droid_net.py:83-109: corr_encoder[2:4],
 * flow_encoder[2:4], delta[0:2], weight[0:2], agg.conv1 and agg.conv2 with their ReLUs), inference only.  The
 * conventions, the library (libdroid_backends_hip.so), DROID_ABI_VERSION and the status codes are those of
 * droid_backends_hip.h.  Binding table: droid_backends/_lib.py ABI_CONV3X3 (tests/test_conv3x3_abi.py holds it against
 * the prototypes here).
 *
 *   y[b,n,v,u] = act( half( sum_{c,ky,kx} x[b,c,v+ky-1,u+kx-1] * w16[n,c,ky,kx]  +  float(b16[n]) ) )
 *
 * x is half and is 0 outside the image (padding=1): outside image b, never the neighbouring row's end, never the next
 *   image.  w16 = half(weight), b16 = half(bias), nearest-even, rounded once, when the layer is packed;
 *   weight.reshape(C_out, 9 C_in) has k = 9 c + 3 ky + kx.  act is max(., 0) for relu = 1 (+0 for every value not above
 *   zero; a NaN stays a NaN) and the identity for relu = 0.
 * Sizes: c_in a multiple of 32 in [32, 512]; c_out a multiple of 64 in [64, 256]; H, W >= 1 and H * W <= 2^30; B in
 *   [0, 65535], B = 0 launches nothing and returns DROID_OK.
 * Arithmetic: every product is exact in fp32; fp32 accumulation (v_mfma_f32_16x16x32_f16), in an order that is fixed
 *   but not specified (it depends on H and W only); then + float(b16[n]) in fp32, ONE rounding to half, then act.  No
 *   atomics: the same bits on every run, and the bits of an image depend neither on B, nor on its position in the
 *   batch, nor on the strides, nor on what ran before.  The kernel writes every LDS byte its matrix operands read.
 *
 * Addressing, 64-bit, in elements (halves):
 *   x[b,c,v,u]  is read at     x + b * x_batch_stride + c * H * W + v * W + u
 *   y[b,n,v,u]  is written at  y + (n / group_channels) * y_group_stride + b * y_batch_stride
 *                                + (n % group_channels) * H * W + v * W + u
 *   so x and y may be channel slices of wider tensors, and one launch over a stacked weight (c_out = 256,
 *   group_channels = 128) writes two separate [B,128,H,W] tensors.  group_channels is a multiple of 64 that divides
 *   c_out; with group_channels == c_out y_group_stride is not used.  x and y need 2-byte alignment only; 16-byte
 *   loads (stores) are used where W is a multiple of 8 and the pointer and the strides of x (of y) are multiples of 8
 *   halves.  Both paths give the same bits.  y must not overlap x: the host cannot see it, the caller answers for it.
 *
 * packed: the parameters of one layer (or of layers stacked along c_out), packed once per network; 16-byte aligned.
 *   halves [c_in / 32 slabs][9 taps][c_out / 16 channel tiles][64 lanes][8], then b16 [c_out]; no padding.
 *   Element (s, t, nt, lane, j) is w16[16 nt + (lane & 15)][32 s + 8 (lane >> 4) + j][t / 3][t % 3]: every weight
 *   appears exactly once.  droid_conv3x3_packed_bytes is host arithmetic, (9 c_in c_out + c_out) * 2, and 0 for sizes
 *   the call refuses.
 *
 * Refusals, DROID_E_ARG with a message that names conv3x3 and the argument, before any HIP call, sizes before pointers,
 * in this order: B ; c_in ; c_out ; H, W ; group_channels ; relu not in {0, 1} ; for B > 1, x_batch_stride below
 * c_in * H * W or y_batch_stride below group_channels * H * W ; then, for B > 0: a null x, packed or y ; a packed that
 * is not 16-byte aligned.  There is no fallback: the framework's convolution stays available.
 */
#ifndef DROID_CONV3X3_HIP_H
#define DROID_CONV3X3_HIP_H

#include "droid_backends_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t droid_conv3x3_packed_bytes(int c_in, int c_out);
int droid_conv3x3(const void* x, const void* packed, void* y, int B, int c_in, int c_out, int H, int W,
                  int64_t x_batch_stride, int64_t y_batch_stride, int64_t y_group_stride, int group_channels, int relu,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DROID_CONV3X3_HIP_H */
