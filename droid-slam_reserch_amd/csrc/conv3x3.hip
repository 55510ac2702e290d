// conv3x3.hip -- Conv2d(C_in, C_out, 3, padding=1) + optional ReLU on half channel-first planes, fp32 accumulation on
// v_mfma_f32_16x16x32_f16 (include/droid_conv3x3_hip.h).  The GEMM of one image: M = pixels, N = C_out, K = 9 C_in,
// walked as C_in / 32 channel slabs x 9 taps, one MFMA K step (32 channels of one tap) at a time.
//
//   Tile.  A workgroup owns TH x TW pixels of one image, 256 of them as 4 x 64, 8 x 32 or 16 x 16 (the host takes the
//     shape that covers the map with the fewest tiles), against 64 CG output channels.  A wave owns 128 of the pixels
//     (8 MFMA pixel tiles) against 64 channels (4 channel tiles): 32 accumulators of 4 floats.  The workgroup is 2 pixel
//     groups x CG channel groups of waves, CG = 2 where C_out is a multiple of 128, else 1.
//   A operand.  An MFMA row wants 8 consecutive K values of one pixel, the input is channel-first: the slab goes through
//     LDS transposed, patch[(TH + 2) x (TW + 2) positions][32 channels] with a pitch of 40 halves, halo included, and
//     everything outside the image is a zero of the kernel's own: the padding is real, in two dimensions.  A fragment of
//     tap (ky, kx) is one 16-byte LDS read at the pixel's position + ky (TW + 2) + kx.  A thread stages 8 pixels of two
//     neighbouring channels (two 16-byte loads where W, the pointer and the batch stride allow it, element loads
//     otherwise) as eight 4-byte LDS writes; the halo columns are element loads.  The loads of the next slab are issued
//     before the MFMAs of the current one and wait in registers.
//   B operand.  The packed weights hold every (slab, tap, channel tile) fragment as 64 lanes x 16 bytes; a wave reads
//     its four fragments of a step straight from L2 / L1.  A fragment serves 8 pixel tiles, and the two waves of a
//     channel group read the same ones: 1 KB from the cache per 8 MFMAs.  (profiles/conv3x3_ab.txt: against weights
//     staged through LDS.)
//   Epilogue.  The pixel mapping of encode_tile.hpp: a lane holds 16 consecutive pixels of a row for each of its
//     channels; ce_store_run adds the bias, rounds once and stores them.
// The loader, the patch and the MFMA loop are conv3x3_core.hpp's, shared with the ConvGRU's gate kernels (gru.hip).
// LDS: every staged position (all rows, the TW columns and both halo columns) x 32 channels is rewritten for every
// slab; the 8 pitch-padding halves of a position are never read.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/droid_conv3x3_hip.h"
#include "conv3x3_core.hpp"
#include "launchers.hpp"

namespace droid {

struct Conv3x3Args {
  C3Segs x;   // one segment
  const f16x8* wpk;
  const __half* b16;
  __half* y;
  int64_t ybs, ygs;
  int c_in, c_out, gch, H, W, tiles_x, relu;
  bool wide_out;
};

template <int TH, int TW, int CG, bool WIDE>
__global__ __launch_bounds__(128 * CG) void conv3x3_kernel(const Conv3x3Args a) {
  constexpr int NTHR = 128 * CG;
  using S = C3Shape<TH, TW, NTHR>;
  __shared__ __attribute__((aligned(16))) _Float16 patch[S::PATCH];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pg = wave & 1, cg = wave >> 1;
  const int H = a.H, W = a.W;
  const size_t HW = (size_t)H * W;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int v0 = ty * TH, u0 = tx * TW;
  const int b = blockIdx.y;
  const int nt0 = (blockIdx.z * CG + cg) * 4;   // the wave's first channel tile
  const int g = lane >> 4, c16 = lane & 15;
  f32x4 acc[4][8];   // [channel tile][pixel tile]
  C3_ACCUMULATE(acc, a.x, a.wpk, a.c_in / C3_SLAB, a.c_out / 16, nt0)

  // ---- epilogue: lane (g, c16) holds, for channel 16 (nt0 + j) + c16, tile pixels 128 pg + 64 h + 16 g + 4 t + i
  __half* yb = a.y + (int64_t)b * a.ybs;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int q0 = 128 * pg + 64 * h + 16 * g;
    const int v = v0 + q0 / TW, u = u0 + q0 % TW;
    if (v >= H || u >= W) continue;
    const int valid = min(16, W - u);   // wide: W % 8 == 0 and u % 16 == 0, so 8 or 16
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int n = 16 * (nt0 + j) + c16;
      const int grp = n / a.gch;
      __half* o = yb + (int64_t)grp * a.ygs + (size_t)(n - grp * a.gch) * HW + (size_t)v * W + u;
      ce_store_run(&acc[j][4 * h], __half2float(a.b16[n]), o, valid, a.wide_out, a.relu != 0);
    }
  }
}

template <int TH, int TW, int CG>
static void c3_launch(const Conv3x3Args& a, int B, bool wide_in, hipStream_t s) {
  const int tiles_y = (a.H + TH - 1) / TH;   // H * W <= 2^30 and 256 pixels per tile: fewer than 2^31 tiles
  const dim3 grid(a.tiles_x * tiles_y, B, a.c_out / (64 * CG));
  if (wide_in) hipLaunchKernelGGL((conv3x3_kernel<TH, TW, CG, true>), grid, dim3(128 * CG), 0, s, a);
  else hipLaunchKernelGGL((conv3x3_kernel<TH, TW, CG, false>), grid, dim3(128 * CG), 0, s, a);
}

template <int CG>
static void c3_launch_shape(Conv3x3Args& a, int B, bool wide_in, hipStream_t s) {
  const int shape = c3_pick_shape(a.H, a.W);
  if (shape == 0) {
    a.tiles_x = (a.W + 63) / 64;
    c3_launch<4, 64, CG>(a, B, wide_in, s);
  } else if (shape == 1) {
    a.tiles_x = (a.W + 31) / 32;
    c3_launch<8, 32, CG>(a, B, wide_in, s);
  } else {
    a.tiles_x = (a.W + 15) / 16;
    c3_launch<16, 16, CG>(a, B, wide_in, s);
  }
}

// every argument has been checked by droid_conv3x3
void launch_conv3x3(const void* x, const void* packed, void* y, int B, int c_in, int c_out, int H, int W,
                    int64_t x_batch_stride, int64_t y_batch_stride, int64_t y_group_stride, int group_channels, int relu,
                    hipStream_t s) {
  Conv3x3Args a;
  a.x = c3_one_segment(x, x_batch_stride, c_in);
  a.wpk = static_cast<const f16x8*>(packed);
  a.b16 = static_cast<const __half*>(packed) + (size_t)9 * c_in * c_out;
  a.y = static_cast<__half*>(y);
  a.ybs = y_batch_stride; a.ygs = group_channels == c_out ? 0 : y_group_stride;
  a.c_in = c_in; a.c_out = c_out; a.gch = group_channels; a.H = H; a.W = W; a.tiles_x = 0; a.relu = relu;
  const bool w8 = (W & 7) == 0;
  const bool wide_in = w8 && c3_segments_wide(a.x, B);
  a.wide_out = w8 && (reinterpret_cast<uintptr_t>(y) & 15) == 0 && (B == 1 || (a.ybs & 7) == 0) && (a.ygs & 7) == 0;
  if (c_out % 128 == 0) c3_launch_shape<2>(a, B, wide_in, s);
  else c3_launch_shape<1>(a, B, wide_in, s);
}

}  // namespace droid
