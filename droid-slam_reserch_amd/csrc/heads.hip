// heads.hip -- the output heads of the update operator: a Conv2d(128, n_out, 3, padding=1) with n_out in {1, 2} under
// autocast, the activation on the fp32 sum and the [B,H,W,n_out] half layout, for one or two heads in one launch
// (include/droid_heads_hip.h).
//
// About 2300 multiply-adds and 256 bytes per pixel and head: the kernel is laid out around the staging of x, and the
// arithmetic is plain fp32 FMAs with the weights on the scalar path.
//   Tile.  A workgroup of four waves owns 4 rows x 64 columns of one batch element of one head.  Every lane owns four
//     consecutive pixels of a row (16 lanes per row), so a 3-tap row of a channel is six halves that serve 12 * n_out
//     FMAs.  The four waves split the 128 channels, 32 each, and meet once, at the end: at the frontend's sizes (24
//     edges of 48 x 64) this is what gives every SIMD of the chip a wave or two.
//   Staging.  A wave stages its own channels, 8 at a time: 6 rows (the 4 and a halo row above and below) x 66 columns
//     (64 and a halo column left and right) per channel.  The 64 columns go as 16-byte loads and 16-byte LDS writes
//     where W is a multiple of 8 and x is 16-byte aligned (UH_WIDE), as element loads otherwise; the halo columns are
//     element loads.  Everything outside the image is a zero of the kernel's own.  The loads of the next 8 channels
//     are issued before the FMAs of the current 8 and wait in registers.
//   Weights.  packed holds float(w16) as [c][ky][kx][n]: the 9 * n_out weights of a channel are one run, addressed by
//     wave-uniform values only, so they are scalar loads and the FMAs take them as scalar operands.
//   End.  The four partial sums of a pixel are added in wave order (fixed), then the bias, the activation in fp32,
//     ONE rounding to half and a store of 4 * n_out halves per lane (one 16- or 8-byte store where W is a multiple of 4
//     and out is aligned, element stores otherwise).
// LDS: every byte a lane reads is written by this launch -- the staging area is cleared once (columns 6 and 73 of a row
// are read next to the halo and never staged), then every staged position is rewritten per channel group.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/droid_heads_hip.h"
#include "launchers.hpp"

namespace droid {

constexpr int UH_C = 128;                 // input channels
constexpr int UH_WAVES = 4;               // waves of a workgroup: each sums UH_C / UH_WAVES channels
constexpr int UH_CG = 8;                  // channels staged at a time by a wave
constexpr int UH_STAGES = UH_C / UH_WAVES / UH_CG;
constexpr int UH_ROWS = 4, UH_COLS = 64;  // the pixel tile
constexpr int UH_SR = UH_ROWS + 2;        // staged rows
constexpr int UH_PITCH = 80;              // halves per staged row: image column u0 + i at 8 + i, halo at 7 and 72
constexpr int UH_AREA = UH_CG * UH_SR * UH_PITCH;   // halves of a wave's staging area
constexpr int UH_SEGS = UH_CG * UH_SR * (UH_COLS / 8);   // 16-byte segments of a channel group: 384, six per lane
constexpr int UH_HALO = UH_CG * UH_SR * 2;               // halo elements of a channel group: 96
static_assert(UH_SEGS == 6 * 64 && UH_HALO <= 2 * 64 && UH_AREA % 8 == 0, "the task lists of uh_load / uh_write");

struct HeadsArgs {
  const __half *x0, *x1;
  const float *p0, *p1;
  __half *o0, *o1;
  int n0, n1, act0, act1;
  int H, W, tiles_x;
};

struct UhRegs {
  uint4 seg[6];
  unsigned short halo[2];
};

// the loads of channel group [c0, c0 + 8) of the tile whose first staged row is image row r0 (may be -1) and whose first
// column is u0; xb = x + b * 128 * HW
template <bool WIDE>
__device__ __forceinline__ void uh_load(UhRegs& g, const __half* __restrict__ xb, int c0, int lane, int r0, int u0, int H,
                                        int W, size_t HW) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const int t = lane + 64 * i;
    const int ch = t / 48, rem = t - 48 * ch, row = rem >> 3, s = rem & 7;
    const int r = r0 + row, u = u0 + 8 * s;
    uint4 v = {0u, 0u, 0u, 0u};
    if (r >= 0 && r < H && u < W) {
      const __half* src = xb + (size_t)(c0 + ch) * HW + (size_t)r * W + u;
      if constexpr (WIDE) {
        v = *reinterpret_cast<const uint4*>(src);   // W % 8 == 0: a segment that begins inside the row ends inside it
      } else {
        const unsigned short* e = reinterpret_cast<const unsigned short*>(src);
        unsigned int h[8];
#pragma unroll
        for (int j = 0; j < 8; j++) h[j] = u + j < W ? e[j] : 0u;
        v.x = h[0] | (h[1] << 16);
        v.y = h[2] | (h[3] << 16);
        v.z = h[4] | (h[5] << 16);
        v.w = h[6] | (h[7] << 16);
      }
    }
    g.seg[i] = v;
  }
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int t = lane + 64 * j;
    const int ch = t / 12, rem = t - 12 * ch, row = rem >> 1, side = rem & 1;
    const int r = r0 + row, u = side ? u0 + UH_COLS : u0 - 1;
    unsigned short v = 0;
    if (t < UH_HALO && r >= 0 && r < H && u >= 0 && u < W)
      v = reinterpret_cast<const unsigned short*>(xb)[(size_t)(c0 + ch) * HW + (size_t)r * W + u];
    g.halo[j] = v;
  }
}

__device__ __forceinline__ void uh_write(const UhRegs& g, _Float16* area, int lane) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const int t = lane + 64 * i;
    const int ch = t / 48, rem = t - 48 * ch, row = rem >> 3, s = rem & 7;
    *reinterpret_cast<uint4*>(area + (ch * UH_SR + row) * UH_PITCH + 8 + 8 * s) = g.seg[i];
  }
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int t = lane + 64 * j;
    const int ch = t / 12, rem = t - 12 * ch, row = rem >> 1, side = rem & 1;
    if (t < UH_HALO)
      reinterpret_cast<unsigned short*>(area)[(ch * UH_SR + row) * UH_PITCH + (side ? 8 + UH_COLS : 7)] = g.halo[j];
  }
}

__device__ __forceinline__ float uh_f(unsigned int bits16) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)bits16);
}

__device__ __forceinline__ float uh_act(int act, float t) {
  if (act == DROID_HEAD_SIGMOID) return 1.0f / (1.0f + expf(-t));
  if (act == DROID_HEAD_SOFTPLUS_CENTI) return 0.01f * (t > 20.0f ? t : log1pf(expf(t)));
  return t;
}

template <int NOUT, bool WIDE>
__device__ __forceinline__ void uh_body(const __half* __restrict__ x, const float* __restrict__ packed,
                                        __half* __restrict__ out, int act, int H, int W, int tiles_x,
                                        _Float16* stage, float* red) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t HW = (size_t)H * W;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int v0 = ty * UH_ROWS, u0 = tx * UH_COLS;
  const __half* xb = x + (size_t)blockIdx.y * UH_C * HW;
  _Float16* area = stage + wave * UH_AREA;
  const int cw = wave * (UH_C / UH_WAVES);   // the wave's first channel

  UhRegs g;
  uh_load<WIDE>(g, xb, cw, lane, v0 - 1, u0, H, W, HW);
  {  // the staging area starts as zeros of the kernel's own
    const uint4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < (UH_AREA / 8 + 63) / 64; i++)
      if (lane + 64 * i < UH_AREA / 8) reinterpret_cast<uint4*>(area)[lane + 64 * i] = z;
  }
  __syncthreads();

  const int lr = lane >> 4, q = lane & 15;
  float acc[4][NOUT];
#pragma unroll
  for (int p = 0; p < 4; p++)
#pragma unroll
    for (int n = 0; n < NOUT; n++) acc[p][n] = 0.f;

#pragma unroll 1
  for (int s = 0; s < UH_STAGES; s++) {
    uh_write(g, area, lane);
    if (s + 1 < UH_STAGES) uh_load<WIDE>(g, xb, cw + (s + 1) * UH_CG, lane, v0 - 1, u0, H, W, HW);
    __syncthreads();   // the group is staged
    const float* wg = packed + (size_t)(cw + s * UH_CG) * 9 * NOUT;
#pragma unroll
    for (int ch = 0; ch < UH_CG; ch++) {
#pragma unroll
      for (int ky = 0; ky < 3; ky++) {
        // columns 6 .. 13 of the lane's window start: image columns u - 2 .. u + 5 of its first pixel u
        const _Float16* rp = area + (ch * UH_SR + lr + ky) * UH_PITCH + 6 + 4 * q;
        const unsigned int lo = *reinterpret_cast<const unsigned int*>(rp);
        const uint2 mid = *reinterpret_cast<const uint2*>(rp + 2);
        const unsigned int hi = *reinterpret_cast<const unsigned int*>(rp + 6);
        const float f[6] = {uh_f(lo >> 16),      uh_f(mid.x & 0xffffu), uh_f(mid.x >> 16),
                            uh_f(mid.y & 0xffffu), uh_f(mid.y >> 16),     uh_f(hi & 0xffffu)};   // columns u - 1 .. u + 4
#pragma unroll
        for (int kx = 0; kx < 3; kx++)
#pragma unroll
          for (int n = 0; n < NOUT; n++) {
            const float w = wg[((ch * 3 + ky) * 3 + kx) * NOUT + n];
#pragma unroll
            for (int p = 0; p < 4; p++) acc[p][n] = fmaf(f[p + kx], w, acc[p][n]);
          }
      }
    }
    __syncthreads();   // the group has been read
  }

  // ---- the four partial sums meet: red[wave][value][lane]
#pragma unroll
  for (int p = 0; p < 4; p++)
#pragma unroll
    for (int n = 0; n < NOUT; n++) red[(wave * 8 + p * NOUT + n) * 64 + lane] = acc[p][n];
  __syncthreads();
  if (wave != 0) return;
  const int v = v0 + lr, u = u0 + 4 * q;
  if (v >= H || u >= W) return;
  unsigned short hb[4][NOUT];
#pragma unroll
  for (int p = 0; p < 4; p++)
#pragma unroll
    for (int n = 0; n < NOUT; n++) {
      const int k = p * NOUT + n;
      float t = red[(0 * 8 + k) * 64 + lane];
#pragma unroll
      for (int w = 1; w < UH_WAVES; w++) t += red[(w * 8 + k) * 64 + lane];
      t += packed[1152 * NOUT + n];
      hb[p][n] = __builtin_bit_cast(unsigned short, __float2half_rn(uh_act(act, t)));
    }
  __half* dst = out + ((size_t)blockIdx.y * HW + (size_t)v * W + u) * NOUT;
  const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;   // then u + 4 <= W and dst is aligned
  if (vec) {
    if constexpr (NOUT == 2) {
      uint4 o;
      o.x = hb[0][0] | ((unsigned int)hb[0][1] << 16);
      o.y = hb[1][0] | ((unsigned int)hb[1][1] << 16);
      o.z = hb[2][0] | ((unsigned int)hb[2][1] << 16);
      o.w = hb[3][0] | ((unsigned int)hb[3][1] << 16);
      *reinterpret_cast<uint4*>(dst) = o;
    } else {
      uint2 o;
      o.x = hb[0][0] | ((unsigned int)hb[1][0] << 16);
      o.y = hb[2][0] | ((unsigned int)hb[3][0] << 16);
      *reinterpret_cast<uint2*>(dst) = o;
    }
  } else {
#pragma unroll
    for (int p = 0; p < 4; p++)
      if (u + p < W)
#pragma unroll
        for (int n = 0; n < NOUT; n++) reinterpret_cast<unsigned short*>(dst)[p * NOUT + n] = hb[p][n];
  }
}

template <bool WIDE>
__global__ __launch_bounds__(64 * UH_WAVES) void update_heads_kernel(const HeadsArgs a) {
  __shared__ __attribute__((aligned(16))) _Float16 stage[UH_WAVES * UH_AREA];
  __shared__ float red[UH_WAVES * 8 * 64];
  const bool second = blockIdx.z != 0;   // wave-uniform: the head's pointers stay on the scalar path
  const __half* x = second ? a.x1 : a.x0;
  const float* packed = second ? a.p1 : a.p0;
  __half* out = second ? a.o1 : a.o0;
  const int n_out = second ? a.n1 : a.n0, act = second ? a.act1 : a.act0;
  if (n_out == 2) uh_body<2, WIDE>(x, packed, out, act, a.H, a.W, a.tiles_x, stage, red);
  else uh_body<1, WIDE>(x, packed, out, act, a.H, a.W, a.tiles_x, stage, red);
}

// every argument has been checked by droid_update_heads
void launch_update_heads(const void* const* x, const void* const* packed, void* const* out, const int* n_out,
                         const int* act, int heads, int B, int H, int W, hipStream_t s) {
  HeadsArgs a;
  const int k1 = heads - 1;   // a call with one head names it twice; the grid has no second slice
  a.x0 = static_cast<const __half*>(x[0]); a.x1 = static_cast<const __half*>(x[k1]);
  a.p0 = static_cast<const float*>(packed[0]); a.p1 = static_cast<const float*>(packed[k1]);
  a.o0 = static_cast<__half*>(out[0]); a.o1 = static_cast<__half*>(out[k1]);
  a.n0 = n_out[0]; a.n1 = n_out[k1];
  a.act0 = act[0]; a.act1 = act[k1];
  a.H = H; a.W = W;
  a.tiles_x = (W + UH_COLS - 1) / UH_COLS;
  const int tiles_y = (H + UH_ROWS - 1) / UH_ROWS;   // H * W <= 2^30: at most 2^28 tiles
  bool wide = (W & 7) == 0;
  for (int k = 0; k < heads; k++) wide = wide && (reinterpret_cast<uintptr_t>(x[k]) & 15) == 0;
  const dim3 grid(a.tiles_x * tiles_y, B, heads);
  if (wide) hipLaunchKernelGGL(update_heads_kernel<true>, grid, dim3(64 * UH_WAVES), 0, s, a);
  else hipLaunchKernelGGL(update_heads_kernel<false>, grid, dim3(64 * UH_WAVES), 0, s, a);
}

}  // namespace droid
