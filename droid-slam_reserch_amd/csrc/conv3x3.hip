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
// LDS: every staged position (all rows, the TW columns and both halo columns) x 32 channels is rewritten for every
// slab; the 8 pitch-padding halves of a position are never read.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/droid_conv3x3_hip.h"
#include "encode_tile.hpp"
#include "launchers.hpp"

namespace droid {

constexpr int C3_SLAB = 32;    // channels of a slab: one MFMA K step per tap
constexpr int C3_PITCH = 40;   // halves per patch position: 32 channels + 8 (16-byte aligned, rows 80 bytes apart)
constexpr int C3_PAIRS = C3_SLAB / 2;

struct Conv3x3Args {
  const __half* x;
  const f16x8* wpk;
  const __half* b16;
  __half* y;
  int64_t xbs, ybs, ygs;
  int c_in, c_out, gch, H, W, tiles_x, relu;
  bool wide_out;
};

template <int TH, int TW, int NTHR>
struct C3Shape {
  static constexpr int PR = TH + 2, PC = TW + 2, SEGS = TW / 8;
  static constexpr int SEG_TASKS = C3_PAIRS * PR * SEGS, HALO_TASKS = C3_PAIRS * PR * 2;
  static constexpr int SEG_IT = (SEG_TASKS + NTHR - 1) / NTHR, HALO_IT = (HALO_TASKS + NTHR - 1) / NTHR;
  static_assert(TH * TW == 256 && TW % 16 == 0, "256 pixels, a lane's 16 pixels inside one row");
};

template <int SEG_IT, int HALO_IT>
struct C3Regs {
  uint4 s0[SEG_IT], s1[SEG_IT];   // 8 pixels of channel 2 cp and of channel 2 cp + 1
  unsigned int halo[HALO_IT];     // one halo position of both channels
};

// the loads of slab `slab` of the tile whose first staged row is image row r0 (may be -1) and first staged column is
// image column u0 - 1; xb = x + b * x_batch_stride
template <typename S, bool WIDE, int NTHR>
__device__ __forceinline__ void c3_load(C3Regs<S::SEG_IT, S::HALO_IT>& g, const __half* __restrict__ xb, int slab, int tid,
                                        int r0, int u0, int H, int W, size_t HW) {
  const unsigned short* xs = reinterpret_cast<const unsigned short*>(xb) + (size_t)slab * C3_SLAB * HW;
#pragma unroll
  for (int it = 0; it < S::SEG_IT; it++) {
    const int t = tid + NTHR * it;
    const int seg = t % S::SEGS, cp = (t / S::SEGS) % C3_PAIRS, row = t / (S::SEGS * C3_PAIRS);
    const int r = r0 + row, u = u0 + 8 * seg;
    uint4 v0 = {0u, 0u, 0u, 0u}, v1 = {0u, 0u, 0u, 0u};
    if (t < S::SEG_TASKS && r >= 0 && r < H && u < W) {
      const unsigned short* src = xs + (size_t)(2 * cp) * HW + (size_t)r * W + u;
      if constexpr (WIDE) {   // W % 8 == 0: a segment that begins inside the row ends inside it
        v0 = *reinterpret_cast<const uint4*>(src);
        v1 = *reinterpret_cast<const uint4*>(src + HW);
      } else {
        unsigned int h0[8], h1[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
          h0[j] = u + j < W ? src[j] : 0u;
          h1[j] = u + j < W ? src[HW + j] : 0u;
        }
        v0.x = h0[0] | (h0[1] << 16); v0.y = h0[2] | (h0[3] << 16); v0.z = h0[4] | (h0[5] << 16); v0.w = h0[6] | (h0[7] << 16);
        v1.x = h1[0] | (h1[1] << 16); v1.y = h1[2] | (h1[3] << 16); v1.z = h1[4] | (h1[5] << 16); v1.w = h1[6] | (h1[7] << 16);
      }
    }
    g.s0[it] = v0;
    g.s1[it] = v1;
  }
#pragma unroll
  for (int it = 0; it < S::HALO_IT; it++) {
    const int t = tid + NTHR * it;
    const int side = t & 1, cp = (t >> 1) % C3_PAIRS, row = t / (2 * C3_PAIRS);
    const int r = r0 + row, u = side ? u0 + S::PC - 2 : u0 - 1;
    unsigned int v = 0u;
    if (t < S::HALO_TASKS && r >= 0 && r < H && u >= 0 && u < W) {
      const unsigned short* src = xs + (size_t)(2 * cp) * HW + (size_t)r * W + u;
      v = src[0] | ((unsigned int)src[HW] << 16);
    }
    g.halo[it] = v;
  }
}

template <typename S, int NTHR>
__device__ __forceinline__ void c3_write(const C3Regs<S::SEG_IT, S::HALO_IT>& g, _Float16* patch, int tid) {
  unsigned int* p32 = reinterpret_cast<unsigned int*>(patch);
#pragma unroll
  for (int it = 0; it < S::SEG_IT; it++) {
    const int t = tid + NTHR * it;
    const int seg = t % S::SEGS, cp = (t / S::SEGS) % C3_PAIRS, row = t / (S::SEGS * C3_PAIRS);
    if (t < S::SEG_TASKS) {
      unsigned int* d = p32 + (row * S::PC + 1 + 8 * seg) * (C3_PITCH / 2) + cp;
      const unsigned int a[4] = {g.s0[it].x, g.s0[it].y, g.s0[it].z, g.s0[it].w};
      const unsigned int b[4] = {g.s1[it].x, g.s1[it].y, g.s1[it].z, g.s1[it].w};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        d[(2 * j) * (C3_PITCH / 2)] = (a[j] & 0xffffu) | (b[j] << 16);
        d[(2 * j + 1) * (C3_PITCH / 2)] = (a[j] >> 16) | (b[j] & 0xffff0000u);
      }
    }
  }
#pragma unroll
  for (int it = 0; it < S::HALO_IT; it++) {
    const int t = tid + NTHR * it;
    const int side = t & 1, cp = (t >> 1) % C3_PAIRS, row = t / (2 * C3_PAIRS);
    if (t < S::HALO_TASKS) p32[(row * S::PC + (side ? S::PC - 1 : 0)) * (C3_PITCH / 2) + cp] = g.halo[it];
  }
}

template <int TH, int TW, int CG, bool WIDE>
__global__ __launch_bounds__(128 * CG) void conv3x3_kernel(const Conv3x3Args a) {
  constexpr int NTHR = 128 * CG;
  using S = C3Shape<TH, TW, NTHR>;
  __shared__ __attribute__((aligned(16))) _Float16 patch[S::PR * S::PC * C3_PITCH];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pg = wave & 1, cg = wave >> 1;
  const int H = a.H, W = a.W;
  const size_t HW = (size_t)H * W;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int v0 = ty * TH, u0 = tx * TW;
  const int b = blockIdx.y;
  const __half* xb = a.x + (int64_t)b * a.xbs;
  const int slabs = a.c_in / C3_SLAB, ntt = a.c_out / 16;
  const int nt0 = (blockIdx.z * CG + cg) * 4;   // the wave's first channel tile

  const int g = lane >> 4, c16 = lane & 15;
  int base[2];   // patch position of tap (0, 0) of the lane's A row in pixel tiles 0 and 4 (+ 4 per tile in between)
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int q = 128 * pg + 64 * h + ce_arow(c16);
    base[h] = (q / TW) * S::PC + q % TW;
  }
  f32x4 acc[4][8];   // [channel tile][pixel tile]
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int t = 0; t < 8; t++) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  C3Regs<S::SEG_IT, S::HALO_IT> regs;
  c3_load<S, WIDE, NTHR>(regs, xb, 0, tid, v0 - 1, u0, H, W, HW);
#pragma unroll 1
  for (int s = 0; s < slabs; s++) {
    c3_write<S, NTHR>(regs, patch, tid);
    if (s + 1 < slabs) c3_load<S, WIDE, NTHR>(regs, xb, s + 1, tid, v0 - 1, u0, H, W, HW);
    __syncthreads();   // the slab is staged
    const f16x8* ws = a.wpk + ((size_t)s * 9 * ntt + nt0) * 64 + lane;
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
      const int off = (tap / 3) * S::PC + tap % 3;
      f16x8 bf[4], af[8];
#pragma unroll
      for (int j = 0; j < 4; j++) bf[j] = ws[((size_t)tap * ntt + j) * 64];
#pragma unroll
      for (int t = 0; t < 8; t++)
        af[t] = *reinterpret_cast<const f16x8*>(patch + (base[t >> 2] + 4 * (t & 3) + off) * C3_PITCH + 8 * g);
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int t = 0; t < 8; t++) acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[t], bf[j], acc[j][t], 0, 0, 0);
    }
    __syncthreads();   // the slab has been read
  }

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
  // the tile shape that covers the map with the fewest tiles; a tie goes to the wider one (longer runs per row)
  auto tiles = [&](int th, int tw) { return (int64_t)((a.H + th - 1) / th) * ((a.W + tw - 1) / tw); };
  const int64_t t64 = tiles(4, 64), t32 = tiles(8, 32), t16 = tiles(16, 16);
  if (t64 <= t32 && t64 <= t16) {
    a.tiles_x = (a.W + 63) / 64;
    c3_launch<4, 64, CG>(a, B, wide_in, s);
  } else if (t32 <= t16) {
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
  a.x = static_cast<const __half*>(x);
  a.wpk = static_cast<const f16x8*>(packed);
  a.b16 = static_cast<const __half*>(packed) + (size_t)9 * c_in * c_out;
  a.y = static_cast<__half*>(y);
  a.xbs = x_batch_stride; a.ybs = y_batch_stride; a.ygs = group_channels == c_out ? 0 : y_group_stride;
  a.c_in = c_in; a.c_out = c_out; a.gch = group_channels; a.H = H; a.W = W; a.tiles_x = 0; a.relu = relu;
  const bool w8 = (W & 7) == 0;
  const bool wide_in = w8 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (B == 1 || (a.xbs & 7) == 0);
  a.wide_out = w8 && (reinterpret_cast<uintptr_t>(y) & 15) == 0 && (B == 1 || (a.ybs & 7) == 0) && (a.ygs & 7) == 0;
  if (c_out % 128 == 0) c3_launch_shape<2>(a, B, wide_in, s);
  else c3_launch_shape<1>(a, B, wide_in, s);
}

}  // namespace droid
