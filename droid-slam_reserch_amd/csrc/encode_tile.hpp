// encode_tile.hpp -- what the two fused encoder kernels share (corr_encode_kernel in corr.hip, motion_encode_kernel in
// motion_encode.hip; include/droid_update_hip.h, include/droid_motion_encode_hip.h): the shape of the LDS A tile, the
// MFMA loop of one 64-column K group against its packed weights, and the epilogue of one channel tile.
//
// A tile: [64 pixels][64 K] halves, row pitch 72 (16-byte aligned rows); 49 of the 64 columns of a group carry values
// (a 7 x 7 window), columns 49..63 are zeros the kernel writes itself.  Packed weights: halves
// [4 groups][2 K steps][8 channel tiles][64 lanes][8], then b16 [128].  MFMA tile t takes as its row r the pixel
// 16 (r >> 2) + 4 t + (r & 3), so that a lane's 16 accumulator elements of one channel are 16 CONSECUTIVE pixels: the
// epilogue (bias, one rounding to half, max with 0) stores them with two 16-byte stores, and the four lanes of a channel
// cover the wave's 64 pixels as one contiguous 128-byte segment.  conv3x3_kernel (conv3x3.hip) takes the types, the row
// mapping (ce_arow) and the epilogue with an address of its own (ce_store_run); its tile and weight layout are its own.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace droid {

constexpr int CE_LEVELS = 4, CE_R = 3, CE_K = 49, CE_KP = 64, CE_N = 128, CE_PITCH = 72;
static_assert(CE_K == (2 * CE_R + 1) * (2 * CE_R + 1) && CE_K <= CE_KP && CE_KP + 8 == CE_PITCH, "A tile: 49 of 64 columns");
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// the pixel (row of the A tile) that is row c16 = lane & 15 of MFMA tile 0 (+ 4 t: tile t)
__device__ __forceinline__ int ce_arow(int c16) { return 16 * (c16 >> 2) + (c16 & 3); }

// group l of the packed weights against the A tile: 2 x 4 x 8 v_mfma_f32_16x16x32_f16 (K steps x pixel tiles x channel
// tiles) into acc[channel tile][pixel tile]; g = lane >> 4, arow = ce_arow(lane & 15)
__device__ __forceinline__ void ce_mma(const _Float16* tile, const f16x8* __restrict__ wpk, int l, int lane, int g, int arow,
                                       f32x4 (&acc)[8][4]) {
#pragma unroll
  for (int s = 0; s < 2; s++) {
    f16x8 a[4];
#pragma unroll
    for (int t = 0; t < 4; t++)
      a[t] = *reinterpret_cast<const f16x8*>(tile + (arow + 4 * t) * CE_PITCH + s * 32 + g * 8);
    const f16x8* wl = wpk + ((size_t)(l * 2 + s) * 8) * 64 + lane;
#pragma unroll
    for (int nt = 0; nt < 8; nt++) {
      const f16x8 bf = wl[nt * 64];
#pragma unroll
      for (int t = 0; t < 4; t++) acc[nt][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[t], bf, acc[nt][t], 0, 0, 0);
    }
  }
}

// epilogue of one channel tile: lane (g, c16) holds, for channel n, the pixels p0 + 4 t + i in acc[t][i]
__device__ __forceinline__ void ce_store(const f32x4 (&acc)[4], int n, const __half* __restrict__ b16, __half* __restrict__ y,
                                         int b, int H1W1, int p0, bool wide) {
#pragma clang fp contract(off)  // the fp32 sum, then ONE rounding to half: no mixed-precision folding of the addition
  const float bias = __half2float(b16[n]);
  __half* o = y + ((size_t)b * CE_N + n) * H1W1 + p0;
  unsigned short h[16];
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const __half r = __float2half_rn(acc[t][i] + bias);
      const float rf = __half2float(r);
      // max(., 0) that keeps a NaN: +0 for everything that is not above zero
      h[4 * t + i] = (rf > 0.f || rf != rf) ? __half_as_ushort(r) : (unsigned short)0;
    }
  if (wide) {
    uint4 v0, v1;
    v0.x = h[0] | ((uint32_t)h[1] << 16); v0.y = h[2] | ((uint32_t)h[3] << 16);
    v0.z = h[4] | ((uint32_t)h[5] << 16); v0.w = h[6] | ((uint32_t)h[7] << 16);
    v1.x = h[8] | ((uint32_t)h[9] << 16); v1.y = h[10] | ((uint32_t)h[11] << 16);
    v1.z = h[12] | ((uint32_t)h[13] << 16); v1.w = h[14] | ((uint32_t)h[15] << 16);
    reinterpret_cast<uint4*>(o)[0] = v0;
    reinterpret_cast<uint4*>(o)[1] = v1;
  } else {
#pragma unroll
    for (int k = 0; k < 16; k++)
      if (p0 + k < H1W1) o[k] = __ushort_as_half(h[k]);
  }
}

// ce_store's sibling for a caller with its own addressing (conv3x3_kernel): the same epilogue -- the fp32 sum, ONE
// rounding to half, then max(., 0) where relu -- of 16 consecutive pixels of channel n's row segment that begins at o;
// the first `valid` of them exist.  wide: two 16-byte stores (o 16-byte aligned, valid 8 or 16), else element stores.
__device__ __forceinline__ void ce_store_run(const f32x4* acc, float bias, __half* __restrict__ o, int valid, bool wide,
                                             bool relu) {
#pragma clang fp contract(off)  // as in ce_store
  unsigned short h[16];
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const __half r = __float2half_rn(acc[t][i] + bias);
      const float rf = __half2float(r);
      h[4 * t + i] = (!relu || rf > 0.f || rf != rf) ? __half_as_ushort(r) : (unsigned short)0;
    }
  if (wide) {
    uint4 v0, v1;
    v0.x = h[0] | ((uint32_t)h[1] << 16); v0.y = h[2] | ((uint32_t)h[3] << 16);
    v0.z = h[4] | ((uint32_t)h[5] << 16); v0.w = h[6] | ((uint32_t)h[7] << 16);
    v1.x = h[8] | ((uint32_t)h[9] << 16); v1.y = h[10] | ((uint32_t)h[11] << 16);
    v1.z = h[12] | ((uint32_t)h[13] << 16); v1.w = h[14] | ((uint32_t)h[15] << 16);
    if (valid >= 8) reinterpret_cast<uint4*>(o)[0] = v0;
    if (valid >= 16) reinterpret_cast<uint4*>(o)[1] = v1;
  } else {
#pragma unroll
    for (int k = 0; k < 16; k++)
      if (k < valid) o[k] = __ushort_as_half(h[k]);
  }
}

}  // namespace droid
