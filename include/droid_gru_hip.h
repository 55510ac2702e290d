/*
 * droid_gru_hip.h -- C ABI of the ConvGRU of the update operator (droid_slam/modules/gru.py with h_planes = 128, called
 * as `net = self.gru(net, inp, corr, flow)` in droid_slam/droid_net.py:127), under autocast, inference only.  The
 * conventions, the library (libdroid_backends_hip.so), DROID_ABI_VERSION and the status codes are those of
 * droid_backends_hip.h.  Binding table: droid_backends/_lib.py ABI_GRU (tests/test_conv_gru_abi.py holds it against the
 * prototypes here).
 *
 * x = cat(net, inp...) along the channels is never made: the inputs are a table of nseg segments, seg[0] = net
 * [B,128,H,W], the others the inputs after it, each half [B,seg_channels[k],H,W] read at
 *   seg[k] + b * seg_batch_stride[k] + c * H * W + v * W + u          (64-bit, in halves; channel slices are fine).
 * C = c_in = sum of seg_channels, P = H * W.  All weights and biases are halves, rounded once (nearest-even) when the
 * module is packed: autocast's cast.  x is 0 outside the image (padding = 1).
 *
 *   a[b,n,p]   = sum_c w16[n,c] net[b,c,p] + bw16[n]                      1 x 1, fp32 on v_mfma_f32_16x16x32_f16
 *   glo[b,n]   = (1/P) sum_p sigmoid(a[b,n,p]) net[b,n,p]                 fp32, never rounded to half
 *   g[b,k,n]   = sum_c wkg16[k][n,c] glo[b,c] + bk16[k][n] + bkg16[k][n]  k in {z, r, q} = {0, 1, 2}; fp32 [B,3,128]
 *   s_z, s_r   = conv3x3(x; Wz16 | Wr16) + g[b,z|r,n]                     fp32 accumulation
 *   z16        = half(sigmoid(s_z))                                       ONE rounding
 *   rnet16     = half(sigmoid(s_r) * float(net))                          ONE rounding
 *   s_q        = conv3x3(cat(rnet16, inp...); Wq16) + g[b,q,n]
 *   out        = half((1 - float(z16)) float(net) + float(z16) tanh(s_q)) fp32, two products and a sum that are not
 *                                                                         contracted, ONE rounding
 *
 * g holds both biases of a gate: the convolution epilogues add one fp32 value per (image, channel).  sigmoid(t) is
 * 1 / (1 + expf(-t)); tanh is an fp32 evaluation that is exactly +-1 for large |t|, never NaN for a finite t, with an
 * absolute error of at most 8 * 2^-24.  Every product of the convolutions is exact in fp32 and is accumulated in fp32 in
 * an order that is fixed but not specified (it depends on H and W only).  No atomics: the same bits on every run, and the
 * bits of an image depend neither on B, nor on its position in the batch, nor on the strides, nor on what ran before.
 * The kernels write every LDS byte their matrix operands read.
 *
 * Sizes: the hidden width is 128 (seg_channels[0] == 128); every seg_channels[k] a positive multiple of 32; 2 <= nseg
 *   <= 5; c_in a multiple of 32 in [160, 512]; H, W >= 1 and H * W <= 2^30; B in [0, 65535], B = 0 launches nothing and
 *   returns DROID_OK; batch strides in halves, each at least channels * H * W when B > 1.
 * Alignment: tensors of halves need 2-byte alignment; 16-byte loads (stores) are used for a tensor where W is a multiple
 *   of 8 and its pointer and batch stride are multiples of 8 halves -- for the convolution's input only when every
 *   segment qualifies.  Both paths give the same bits.  g needs 4-byte, ws and packed 16-byte alignment.
 *
 * The phases:
 *   droid_gru_context   g <- net.  ws: scratch of at least B * ceil(P / 256) * 512 bytes (the first part of
 *                       droid_gru_workspace_bytes); two launches.
 *   droid_gru_gates     z [B,128,H,W], rnet [B,128,H,W] (both contiguous halves) <- seg (seg[0] = net), g.
 *   droid_gru_update    out <- seg (seg[0] = rnet, the others as before), g, z, net.  out[b,n,v,u] is written at
 *                       out + b * out_batch_stride + n * H * W + v * W + u.  net is no convolution input of this launch
 *                       and an element of net is read only by the lane that writes the same element of out: out may BE
 *                       net (same pointer and stride).  Any other overlap of out with an input is the caller's fault;
 *                       the host cannot see it.
 *   droid_conv_gru      the three phases in order, seg[0] = net, with g, z and rnet held in ws
 *                       (droid_gru_workspace_bytes(B, H, W) bytes: the context partials, g, z, rnet, each part 16-byte
 *                       aligned); the bits of the phase calls.  out may be seg[0].
 *   droid_gru_packed_bytes and droid_gru_workspace_bytes are host arithmetic and return 0 for sizes the calls refuse.
 *
 * packed: the parameters of one module, packed once per network, halves, 16-byte aligned, no padding, in this order:
 *   [Wz; Wr]  [c_in / 32 slabs][9 taps][16 channel tiles][64 lanes][8]: the fragment layout of droid_conv3x3 for
 *             (c_in, 256) without its bias; element (s, t, nt, lane, j) is W[16 nt + (lane & 15)][32 s + 8 (lane >> 4) + j]
 *             [t / 3][t % 3] of the stacked weight W = cat(convz.weight, convr.weight) rounded to half
 *   Wq        [c_in / 32][9][8][64][8], the same layout for (c_in, 128)
 *   w         [4 slabs][8 channel tiles][64 lanes][8]: element (s, nt, lane, j) = w16[16 nt + (lane & 15)][32 s + 8 (lane >> 4) + j]
 *   wzg, wrg, wqg   [128][128] row-major each (the 1 x 1 weights of convz_glo, convr_glo, convq_glo)
 *   bw, bz, br, bq, bzg, brg, bqg   [128] each
 *   in all (9 * c_in * 384 + 4 * 128 * 128 + 7 * 128) * 2 bytes; every weight appears exactly once.
 *
 * Refusals, DROID_E_ARG with a message that names conv_gru and the argument, before any HIP call, sizes before pointers,
 * in this order: B ; nseg (droid_gru_context: c_in instead of the segment checks) ; a null seg, seg_batch_stride or
 * seg_channels array (they hold the sizes) ; seg_channels[0] != 128 or a seg_channels[k] that is no positive multiple of
 * 32 ; c_in ; H, W ; for B > 1 a seg_batch_stride[k] below seg_channels[k] * H * W, then net_batch_stride, then
 * out_batch_stride below 128 * H * W ; ws_bytes too small ; then, for B > 0: a null pointer (an entry of seg, packed, g,
 * z, rnet, net, out, ws) ; a packed or ws that is not 16-byte aligned.  There is no fallback.
 */
#ifndef DROID_GRU_HIP_H
#define DROID_GRU_HIP_H

#include "droid_backends_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t droid_gru_packed_bytes(int c_in);
size_t droid_gru_workspace_bytes(int B, int H, int W);
int droid_gru_context(const void* net, int64_t net_batch_stride, const void* packed, int c_in, int B, int H, int W,
                      float* g, void* ws, size_t ws_bytes, void* stream);
int droid_gru_gates(const void* const* seg, const int64_t* seg_batch_stride, const int* seg_channels, int nseg,
                    const void* packed, const float* g, void* z, void* rnet, int B, int H, int W, void* stream);
int droid_gru_update(const void* const* seg, const int64_t* seg_batch_stride, const int* seg_channels, int nseg,
                     const void* packed, const float* g, const void* z, const void* net, int64_t net_batch_stride,
                     void* out, int64_t out_batch_stride, int B, int H, int W, void* stream);
int droid_conv_gru(const void* const* seg, const int64_t* seg_batch_stride, const int* seg_channels, int nseg,
                   const void* packed, void* out, int64_t out_batch_stride, int B, int H, int W, void* ws, size_t ws_bytes,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DROID_GRU_HIP_H */
