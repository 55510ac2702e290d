// conv3x3_core.hpp -- what the 3 x 3 convolution kernels share (conv3x3_kernel in conv3x3.hip, the gate kernels in gru.hip):
// the slab loader and its LDS patch, the slab x tap MFMA loop into a wave's 32 accumulators (C3_ACCUMULATE), the pixels a lane holds in
// the epilogue, a store of 16 rounded halves, and the host's choice of the tile shape.  The layout of the tile, of the A
// patch and of the packed weights is described at the top of conv3x3.hip.
//
// The input is a table of at most 5 segments, each {pointer, batch stride, channels, first channel}: the channels of the
// convolution are the segments' channels one after the other (a torch.cat along dim 1 that is never made).  Every
// segment holds a multiple of 32 channels, so a 32-channel slab lies inside one segment; which one is decided once per
// slab, from wave-uniform values.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "encode_tile.hpp"

namespace droid {

constexpr int C3_SLAB = 32;    // channels of a slab: one MFMA K step per tap
constexpr int C3_PITCH = 40;   // halves per patch position: 32 channels + 8 (16-byte aligned, rows 80 bytes apart)
constexpr int C3_PAIRS = C3_SLAB / 2;
constexpr int C3_MAX_SEGS = 5;

struct C3Seg {
  const __half* p;
  int64_t bs;        // batch stride in halves
  int first, end;    // the segment holds the channels first .. end - 1 of the convolution's input
};
struct C3Segs {
  C3Seg s[C3_MAX_SEGS];
  int n;
};

// host: a table of one segment
inline C3Segs c3_one_segment(const void* x, int64_t batch_stride, int channels) {
  C3Segs t = {};
  t.s[0] = C3Seg{static_cast<const __half*>(x), batch_stride, 0, channels};
  t.n = 1;
  return t;
}

// host: whether every segment allows the 16-byte loads (W a multiple of 8 is the caller's to check)
inline bool c3_segments_wide(const C3Segs& t, int B) {
  bool wide = true;
  for (int k = 0; k < t.n; k++) wide = wide && (reinterpret_cast<uintptr_t>(t.s[k].p) & 15) == 0 && (B == 1 || (t.s[k].bs & 7) == 0);
  return wide;
}

// the first half of slab `slab` (channels 32 slab .. 32 slab + 31 of the convolution) in image b
__device__ __forceinline__ const __half* c3_slab_ptr(const C3Segs& t, int slab, int b, size_t HW) {
  const int c = slab * C3_SLAB;
  const __half* p = t.s[0].p;
  int64_t bs = t.s[0].bs;
  int first = 0;
#pragma unroll
  for (int k = 1; k < C3_MAX_SEGS; k++)
    if (k < t.n && c >= t.s[k].first) {
      p = t.s[k].p;
      bs = t.s[k].bs;
      first = t.s[k].first;
    }
  return p + (int64_t)b * bs + (size_t)(c - first) * HW;
}

template <int TH, int TW, int NTHR>
struct C3Shape {
  static constexpr int PR = TH + 2, PC = TW + 2, SEGS = TW / 8;
  static constexpr int SEG_TASKS = C3_PAIRS * PR * SEGS, HALO_TASKS = C3_PAIRS * PR * 2;
  static constexpr int SEG_IT = (SEG_TASKS + NTHR - 1) / NTHR, HALO_IT = (HALO_TASKS + NTHR - 1) / NTHR;
  static constexpr int PATCH = PR * PC * C3_PITCH;   // halves of the LDS patch
  static_assert(TH * TW == 256 && TW % 16 == 0, "256 pixels, a lane's 16 pixels inside one row");
};

template <int SEG_IT, int HALO_IT>
struct C3Regs {
  uint4 s0[SEG_IT], s1[SEG_IT];   // 8 pixels of channel 2 cp and of channel 2 cp + 1
  unsigned int halo[HALO_IT];     // one halo position of both channels
};

// the loads of the slab that begins at xslab (c3_slab_ptr) for the tile whose first staged row is image row r0 (may be
// -1) and first staged column is image column u0 - 1
template <typename S, bool WIDE, int NTHR>
__device__ __forceinline__ void c3_load(C3Regs<S::SEG_IT, S::HALO_IT>& g, const __half* __restrict__ xslab, int tid,
                                        int r0, int u0, int H, int W, size_t HW) {
  const unsigned short* xs = reinterpret_cast<const unsigned short*>(xslab);
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

// The convolution of the workgroup's tile (first pixel (v0, u0) of image b) against the wave's four channel tiles
// nt0 .. nt0 + 3 of the packed weights wpk_ (ntt_ channel tiles in all, slabs_ slabs), into f32x4 acc_[4][8] =
// [channel tile][pixel tile], zeroed here.  Expects in scope: TH, TW, NTHR, WIDE, S = C3Shape<TH, TW, NTHR>, the LDS
// array patch[S::PATCH], and tid, lane, pg, g, c16, b, H, W, HW, v0, u0.  Wave pg + 2 cg owns the pixels 128 pg ..
// 128 pg + 127 of the tile.  A macro and not a function: behind a function boundary (forced inline, the accumulators by
// reference) the compiler allocates 192 instead of 128 AGPRs for the 4 x 64 tile and schedules the fragment reads
// differently, and Conv3x3 is 25 - 45 % slower (profiles/conv_gru_ab.txt).
#define C3_ACCUMULATE(acc_, segs_, wpk_, slabs_, ntt_, nt0_)                                                              \
  int base[2]; /* patch position of tap (0, 0) of the lane's A row in pixel tiles 0 and 4 (+ 4 per tile in between) */ \
  _Pragma("unroll") for (int h = 0; h < 2; h++) {                                                                       \
    const int q = 128 * pg + 64 * h + ce_arow(c16);                                                                     \
    base[h] = (q / TW) * S::PC + q % TW;                                                                                \
  }                                                                                                                     \
  _Pragma("unroll") for (int j = 0; j < 4; j++)                                                                         \
    _Pragma("unroll") for (int t = 0; t < 8; t++) acc_[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};                               \
  C3Regs<S::SEG_IT, S::HALO_IT> regs;                                                                                   \
  c3_load<S, WIDE, NTHR>(regs, c3_slab_ptr(segs_, 0, b, HW), tid, v0 - 1, u0, H, W, HW);                                \
  _Pragma("unroll 1") for (int s = 0; s < (slabs_); s++) {                                                              \
    c3_write<S, NTHR>(regs, patch, tid);                                                                                \
    if (s + 1 < (slabs_)) c3_load<S, WIDE, NTHR>(regs, c3_slab_ptr(segs_, s + 1, b, HW), tid, v0 - 1, u0, H, W, HW);    \
    __syncthreads(); /* the slab is staged */                                                                           \
    const f16x8* ws = (wpk_) + ((size_t)s * 9 * (ntt_) + (nt0_)) * 64 + lane;                                           \
    _Pragma("unroll") for (int tap = 0; tap < 9; tap++) {                                                               \
      const int off = (tap / 3) * S::PC + tap % 3;                                                                      \
      f16x8 bf[4], af[8];                                                                                               \
      _Pragma("unroll") for (int j = 0; j < 4; j++) bf[j] = ws[((size_t)tap * (ntt_) + j) * 64];                        \
      _Pragma("unroll") for (int t = 0; t < 8; t++)                                                                     \
        af[t] = *reinterpret_cast<const f16x8*>(patch + (base[t >> 2] + 4 * (t & 3) + off) * C3_PITCH + 8 * g);         \
      _Pragma("unroll") for (int j = 0; j < 4; j++)                                                                     \
        _Pragma("unroll") for (int t = 0; t < 8; t++)                                                                   \
          acc_[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[t], bf[j], acc_[j][t], 0, 0, 0);                       \
    }                                                                                                                   \
    __syncthreads(); /* the slab has been read */                                                                       \
  }

// (No __restrict__ on the two helpers below: the ConvGRU's blend may write the run it has just read.)
// 16 halves to the row segment that begins at o, the first `valid` of them: two 16-byte stores where wide (o 16-byte
// aligned, valid 8 or 16), element stores otherwise
__device__ __forceinline__ void c3_store16(const unsigned short (&h)[16], __half* o, int valid, bool wide) {
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

// the first `valid` of the 16 halves of the row segment that begins at p, as floats (the others 0); wide as above
__device__ __forceinline__ void c3_load16(float (&f)[16], const __half* p, int valid, bool wide) {
  unsigned short h[16];
  if (wide) {
    uint4 v0 = {0u, 0u, 0u, 0u}, v1 = {0u, 0u, 0u, 0u};
    if (valid >= 8) v0 = reinterpret_cast<const uint4*>(p)[0];
    if (valid >= 16) v1 = reinterpret_cast<const uint4*>(p)[1];
    const unsigned int w[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int k = 0; k < 8; k++) {
      h[2 * k] = (unsigned short)(w[k] & 0xffffu);
      h[2 * k + 1] = (unsigned short)(w[k] >> 16);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; k++) h[k] = k < valid ? reinterpret_cast<const unsigned short*>(p)[k] : (unsigned short)0;
  }
#pragma unroll
  for (int k = 0; k < 16; k++) f[k] = (float)__builtin_bit_cast(_Float16, h[k]);
}

// host: the tile shape that covers the map with the fewest tiles; a tie goes to the wider one (longer runs per row).
// Returns 0 (4 x 64), 1 (8 x 32) or 2 (16 x 16).
inline int c3_pick_shape(int H, int W) {
  auto tiles = [&](int th, int tw) { return (int64_t)((H + th - 1) / th) * ((W + tw - 1) / tw); };
  const int64_t t64 = tiles(4, 64), t32 = tiles(8, 32), t16 = tiles(16, 16);
  if (t64 <= t32 && t64 <= t16) return 0;
  return t32 <= t16 ? 1 : 2;
}

}  // namespace droid
