// gru.hip -- the ConvGRU of the update operator (droid_slam/modules/gru.py, hidden width 128) in four launches
// (include/droid_gru_hip.h states the arithmetic):
//
//   1. gru_context_partial_kernel.  A workgroup owns 256 consecutive pixels of one image (flat, no halo).  It stages the
//      four 32-channel slabs of net transposed through LDS -- conv3x3_core.hpp's patch of 256 positions x 32 channels,
//      pitch 40 -- runs the 128 x 128 1 x 1 convolution on v_mfma_f32_16x16x32_f16 (4 waves = 2 pixel groups x 2 channel
//      groups, a wave 128 pixels x 64 channels, the accumulator mapping of the 3 x 3 kernel), and in its epilogue forms
//      sigmoid(a) * net for the lane's 16 pixels of each channel, masks the pixels past the image and reduces over the
//      tile in a fixed order: a lane's 32 pixels in ascending order, then the 8 (pixel group, g) partials through LDS.
//      It writes [B, tiles, 128] fp32.
//   2. gru_context_finish_kernel.  One workgroup per image: the tile partials in tile order, times 1 / P, then the
//      three 128 x 128 mat-vecs against half weights in fp32 (one thread per output, fmaf in channel order), + both
//      biases of the gate: g [B,3,128].
//   3. gru_gates_kernel.  conv3x3_core.hpp's convolution against the stacked [Wz; Wr] (256 output channels, grid z = 2)
//      over the segments net, inp...; blockIdx.z = 0 writes z16 = half(sigmoid(s + g)), blockIdx.z = 1 loads the lane's
//      16 pixels of net and writes rnet16 = half(sigmoid(s + g) * net).
//   4. gru_update_kernel.  The convolution against Wq over the segments rnet16, inp...; the epilogue loads z16 and net
//      for the lane's run and writes out = half((1 - z) net + z tanh(s + g)).  net is no convolution input of this
//      launch and an element of net is read only by the lane that writes the same element of out: out may be net.
//
// No atomics; every summation order depends on H and W only.  LDS: every patch position is rewritten for every slab
// (zeros past the image), the reduction array is written before it is read.  Vector stores only.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/droid_gru_hip.h"
#include "conv3x3_core.hpp"
#include "launchers.hpp"

namespace droid {

constexpr int GRU_N = 128;                    // the hidden width
constexpr int GRU_CTX_PIX = 256;              // pixels of a context tile

__device__ __forceinline__ float gru_sigmoid(float t) { return 1.0f / (1.0f + expf(-t)); }

// ---------------------------------------------------------------------------------------------- the packed parameters
struct GruPacked {
  const __half *wzr, *wq, *w, *wg, *bias;   // bias: bw, bz, br, bq, bzg, brg, bqg, 128 halves each
};

static GruPacked gru_parts(const void* packed, int c_in) {
  GruPacked p;
  p.wzr = static_cast<const __half*>(packed);
  p.wq = p.wzr + (size_t)9 * c_in * 2 * GRU_N;
  p.w = p.wq + (size_t)9 * c_in * GRU_N;
  p.wg = p.w + GRU_N * GRU_N;
  p.bias = p.wg + 3 * GRU_N * GRU_N;
  return p;
}

size_t gru_packed_bytes(int c_in) { return ((size_t)9 * c_in * 3 * GRU_N + 4 * GRU_N * GRU_N + 7 * GRU_N) * 2; }

static int64_t gru_ctx_tiles(int H, int W) { return ((int64_t)H * W + GRU_CTX_PIX - 1) / GRU_CTX_PIX; }

size_t gru_context_workspace_bytes(int B, int H, int W) { return (size_t)B * gru_ctx_tiles(H, W) * GRU_N * sizeof(float); }

static size_t gru_plane_bytes(int B, int H, int W) { return (((size_t)B * GRU_N * H * W * 2) + 15) & ~(size_t)15; }

size_t gru_workspace_bytes(int B, int H, int W) {
  return gru_context_workspace_bytes(B, H, W) + (size_t)B * 3 * GRU_N * sizeof(float) + 2 * gru_plane_bytes(B, H, W);
}

// ------------------------------------------------------------------------------------------------ 1. context partials
struct GruCtxArgs {
  const __half* net;
  int64_t nbs;
  const f16x8* w;      // [4 slabs][8 channel tiles][64 lanes] fragments
  const __half* bw;
  float* part;         // [B, tiles, 128]
  int P, tiles;
  bool wide;
};

struct GruCtxRegs {
  uint4 s0[2], s1[2];
};

template <bool WIDE>
__device__ __forceinline__ void gru_ctx_load(GruCtxRegs& r, const __half* __restrict__ nb, int slab, int tid, int p0, int P) {
  const unsigned short* xs = reinterpret_cast<const unsigned short*>(nb) + (size_t)slab * C3_SLAB * P;
#pragma unroll
  for (int it = 0; it < 2; it++) {
    const int t = tid + 256 * it;
    const int seg = t & 31, cp = t >> 5;
    const int p = p0 + 8 * seg;
    uint4 v0 = {0u, 0u, 0u, 0u}, v1 = {0u, 0u, 0u, 0u};
    if (p < P) {
      const unsigned short* src = xs + (size_t)(2 * cp) * P + p;
      if constexpr (WIDE) {   // P % 8 == 0: a run that begins inside the image ends inside it
        v0 = *reinterpret_cast<const uint4*>(src);
        v1 = *reinterpret_cast<const uint4*>(src + P);
      } else {
        unsigned int h0[8], h1[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
          h0[j] = p + j < P ? src[j] : 0u;
          h1[j] = p + j < P ? src[(size_t)P + j] : 0u;
        }
        v0.x = h0[0] | (h0[1] << 16); v0.y = h0[2] | (h0[3] << 16); v0.z = h0[4] | (h0[5] << 16); v0.w = h0[6] | (h0[7] << 16);
        v1.x = h1[0] | (h1[1] << 16); v1.y = h1[2] | (h1[3] << 16); v1.z = h1[4] | (h1[5] << 16); v1.w = h1[6] | (h1[7] << 16);
      }
    }
    r.s0[it] = v0;
    r.s1[it] = v1;
  }
}

__device__ __forceinline__ void gru_ctx_write(const GruCtxRegs& r, _Float16* patch, int tid) {
  unsigned int* p32 = reinterpret_cast<unsigned int*>(patch);
#pragma unroll
  for (int it = 0; it < 2; it++) {
    const int t = tid + 256 * it;
    const int seg = t & 31, cp = t >> 5;
    unsigned int* d = p32 + (8 * seg) * (C3_PITCH / 2) + cp;
    const unsigned int a[4] = {r.s0[it].x, r.s0[it].y, r.s0[it].z, r.s0[it].w};
    const unsigned int b[4] = {r.s1[it].x, r.s1[it].y, r.s1[it].z, r.s1[it].w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      d[(2 * j) * (C3_PITCH / 2)] = (a[j] & 0xffffu) | (b[j] << 16);
      d[(2 * j + 1) * (C3_PITCH / 2)] = (a[j] >> 16) | (b[j] & 0xffff0000u);
    }
  }
}

template <bool WIDE>
__global__ __launch_bounds__(256) void gru_context_partial_kernel(const GruCtxArgs a) {
  __shared__ __attribute__((aligned(16))) _Float16 patch[GRU_CTX_PIX * C3_PITCH];
  __shared__ float red[2][4][GRU_N];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pg = wave & 1, cg = wave >> 1;
  const int P = a.P, p0 = blockIdx.x * GRU_CTX_PIX, b = blockIdx.y;
  const __half* nb = a.net + (int64_t)b * a.nbs;
  const int g = lane >> 4, c16 = lane & 15;
  const int nt0 = cg * 4;
  int base[2];
#pragma unroll
  for (int h = 0; h < 2; h++) base[h] = 128 * pg + 64 * h + ce_arow(c16);
  f32x4 acc[4][8];
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int t = 0; t < 8; t++) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  GruCtxRegs regs;
  gru_ctx_load<WIDE>(regs, nb, 0, tid, p0, P);
#pragma unroll 1
  for (int s = 0; s < GRU_N / C3_SLAB; s++) {
    gru_ctx_write(regs, patch, tid);
    if (s + 1 < GRU_N / C3_SLAB) gru_ctx_load<WIDE>(regs, nb, s + 1, tid, p0, P);
    __syncthreads();   // the slab is staged
    const f16x8* ws = a.w + ((size_t)s * 8 + nt0) * 64 + lane;
    f16x8 bf[4], af[8];
#pragma unroll
    for (int j = 0; j < 4; j++) bf[j] = ws[j * 64];
#pragma unroll
    for (int t = 0; t < 8; t++) af[t] = *reinterpret_cast<const f16x8*>(patch + (base[t >> 2] + 4 * (t & 3)) * C3_PITCH + 8 * g);
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int t = 0; t < 8; t++) acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[t], bf[j], acc[j][t], 0, 0, 0);
    __syncthreads();   // the slab has been read
  }

  // lane (g, c16) holds, for channel 16 (nt0 + j) + c16, the tile's pixels 128 pg + 64 h + 16 g + 4 t + i
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int n = 16 * (nt0 + j) + c16;
    const float bias = __half2float(a.bw[n]);
    float sum = 0.f;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int p = p0 + 128 * pg + 64 * h + 16 * g;
      const int valid = min(16, P - p);   // wide: P % 8 == 0 and p % 16 == 0, so 8 or 16 where positive
      if (valid > 0) {
        float x[16];
        c3_load16(x, nb + (size_t)n * P + p, valid, a.wide);
#pragma unroll
        for (int k = 0; k < 16; k++)
          if (k < valid) sum += gru_sigmoid(acc[j][4 * h + (k >> 2)][k & 3] + bias) * x[k];
      }
    }
    red[pg][g][n] = sum;
  }
  __syncthreads();
  if (tid < GRU_N) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
      for (int r = 0; r < 4; r++) s += red[q][r][tid];
    a.part[((size_t)b * a.tiles + blockIdx.x) * GRU_N + tid] = s;
  }
}

// -------------------------------------------------------------------------------------------------- 2. context finish
struct GruFinArgs {
  const float* part;
  const __half *wg, *bias;
  float* g;
  int tiles;
  float inv_p;
};

__global__ __launch_bounds__(3 * GRU_N) void gru_context_finish_kernel(const GruFinArgs a) {
  __shared__ float glo[GRU_N];
  const int tid = threadIdx.x, b = blockIdx.x;
  if (tid < GRU_N) {
    const float* p = a.part + (size_t)b * a.tiles * GRU_N + tid;
    float s = 0.f;
    for (int t = 0; t < a.tiles; t++) s += p[(size_t)t * GRU_N];
    glo[tid] = s * a.inv_p;
  }
  __syncthreads();
  const int k = tid / GRU_N, n = tid - k * GRU_N;
  const uint4* row = reinterpret_cast<const uint4*>(a.wg + ((size_t)k * GRU_N + n) * GRU_N);
  float s = 0.f;
#pragma unroll 4
  for (int c8 = 0; c8 < GRU_N / 8; c8++) {
    const uint4 v = row[c8];
    const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      s = fmaf((float)__builtin_bit_cast(_Float16, (unsigned short)(w[j] & 0xffffu)), glo[8 * c8 + 2 * j], s);
      s = fmaf((float)__builtin_bit_cast(_Float16, (unsigned short)(w[j] >> 16)), glo[8 * c8 + 2 * j + 1], s);
    }
  }
  s = s + __half2float(a.bias[(1 + k) * GRU_N + n]);   // the gate's 3 x 3 bias
  s = s + __half2float(a.bias[(4 + k) * GRU_N + n]);   // the bias of its context matrix
  a.g[((size_t)b * 3 + k) * GRU_N + n] = s;
}

// every argument has been checked by the caller in api.hip
void launch_gru_context(const void* net, int64_t net_batch_stride, const void* packed, int c_in, int B, int H, int W,
                        float* g, void* ws, hipStream_t s) {
  const GruPacked pk = gru_parts(packed, c_in);
  const int P = H * W;
  GruCtxArgs a;
  a.net = static_cast<const __half*>(net);
  a.nbs = net_batch_stride;
  a.w = reinterpret_cast<const f16x8*>(pk.w);
  a.bw = pk.bias;
  a.part = static_cast<float*>(ws);
  a.P = P;
  a.tiles = (int)gru_ctx_tiles(H, W);
  a.wide = (P & 7) == 0 && (reinterpret_cast<uintptr_t>(net) & 15) == 0 && (B == 1 || (net_batch_stride & 7) == 0);
  const dim3 grid(a.tiles, B);
  if (a.wide) hipLaunchKernelGGL(gru_context_partial_kernel<true>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(gru_context_partial_kernel<false>, grid, dim3(256), 0, s, a);
  GruFinArgs f;
  f.part = a.part; f.wg = pk.wg; f.bias = pk.bias; f.g = g; f.tiles = a.tiles; f.inv_p = 1.0f / (float)P;
  hipLaunchKernelGGL(gru_context_finish_kernel, dim3(B), dim3(3 * GRU_N), 0, s, f);
}

// ------------------------------------------------------------------------------------------- 3., 4. the gate kernels
struct GruGateArgs {
  C3Segs x;            // gates: net, inp...; update: rnet16, inp...
  const f16x8* wpk;
  const float* g;      // [B,3,128]
  __half *z, *rnet;    // contiguous [B,128,H,W]; the update reads z
  const __half* net;   // gates: segment 0; update: the hidden state
  int64_t nbs;
  __half* out;
  int64_t obs;
  int slabs, H, W, tiles_x;
  bool wide_zr, wide_net, wide_out;
};

template <int TH, int TW, bool WIDE>
__global__ __launch_bounds__(256) void gru_gates_kernel(const GruGateArgs a) {
  constexpr int NTHR = 256;
  using S = C3Shape<TH, TW, NTHR>;
  __shared__ __attribute__((aligned(16))) _Float16 patch[S::PATCH];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pg = wave & 1, cg = wave >> 1;
  const int H = a.H, W = a.W;
  const size_t HW = (size_t)H * W;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int v0 = ty * TH, u0 = tx * TW;
  const int b = blockIdx.y, gate = blockIdx.z;   // 0: z, 1: r
  const int nt0 = (gate * 2 + cg) * 4;
  const int g = lane >> 4, c16 = lane & 15;
  f32x4 acc[4][8];
  C3_ACCUMULATE(acc, a.x, a.wpk, a.slabs, 2 * GRU_N / 16, nt0)

  const float* gb = a.g + ((size_t)b * 3 + gate) * GRU_N;
  const __half* nb = a.net + (int64_t)b * a.nbs;
  __half* ob = (gate == 0 ? a.z : a.rnet) + (size_t)b * GRU_N * HW;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int q0 = 128 * pg + 64 * h + 16 * g;
    const int v = v0 + q0 / TW, u = u0 + q0 % TW;
    if (v >= H || u >= W) continue;
    const int valid = min(16, W - u);   // wide: W % 8 == 0 and u % 16 == 0, so 8 or 16
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int n = (16 * (nt0 + j) + c16) & (GRU_N - 1);
      const size_t pix = (size_t)n * HW + (size_t)v * W + u;
      const float gv = gb[n];
      unsigned short r[16];
      if (gate == 0) {
#pragma unroll
        for (int k = 0; k < 16; k++) r[k] = __half_as_ushort(__float2half_rn(gru_sigmoid(acc[j][4 * h + (k >> 2)][k & 3] + gv)));
      } else {
        float x[16];
        c3_load16(x, nb + pix, valid, a.wide_net);
#pragma unroll
        for (int k = 0; k < 16; k++)
          r[k] = __half_as_ushort(__float2half_rn(gru_sigmoid(acc[j][4 * h + (k >> 2)][k & 3] + gv) * x[k]));
      }
      c3_store16(r, ob + pix, valid, a.wide_zr);
    }
  }
}

template <int TH, int TW, bool WIDE>
__global__ __launch_bounds__(256) void gru_update_kernel(const GruGateArgs a) {
#pragma clang fp contract(off)   // the blend is two products and a sum in fp32, then ONE rounding to half
  constexpr int NTHR = 256;
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
  const int nt0 = cg * 4;
  const int g = lane >> 4, c16 = lane & 15;
  f32x4 acc[4][8];
  C3_ACCUMULATE(acc, a.x, a.wpk, a.slabs, GRU_N / 16, nt0)

  const float* gb = a.g + ((size_t)b * 3 + 2) * GRU_N;
  const __half* nb = a.net + (int64_t)b * a.nbs;
  const __half* zb = a.z + (size_t)b * GRU_N * HW;
  __half* ob = a.out + (int64_t)b * a.obs;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int q0 = 128 * pg + 64 * h + 16 * g;
    const int v = v0 + q0 / TW, u = u0 + q0 % TW;
    if (v >= H || u >= W) continue;
    const int valid = min(16, W - u);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int n = 16 * (nt0 + j) + c16;
      const size_t pix = (size_t)n * HW + (size_t)v * W + u;
      const float gv = gb[n];
      float z[16], x[16];
      c3_load16(z, zb + pix, valid, a.wide_zr);
      c3_load16(x, nb + pix, valid, a.wide_net);   // read before the store below: out may be net
      unsigned short r[16];
#pragma unroll
      for (int k = 0; k < 16; k++) {
        const float q = tanhf(acc[j][4 * h + (k >> 2)][k & 3] + gv);
        const float keep = (1.0f - z[k]) * x[k];
        const float take = z[k] * q;
        r[k] = __half_as_ushort(__float2half_rn(keep + take));
      }
      c3_store16(r, ob + pix, valid, a.wide_out);
    }
  }
}

template <int TH, int TW>
static void gru_launch(GruGateArgs& a, bool update, int B, bool wide_in, hipStream_t s) {
  a.tiles_x = (a.W + TW - 1) / TW;
  const dim3 grid(a.tiles_x * ((a.H + TH - 1) / TH), B, update ? 1 : 2);
  if (update) {
    if (wide_in) hipLaunchKernelGGL((gru_update_kernel<TH, TW, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((gru_update_kernel<TH, TW, false>), grid, dim3(256), 0, s, a);
  } else {
    if (wide_in) hipLaunchKernelGGL((gru_gates_kernel<TH, TW, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((gru_gates_kernel<TH, TW, false>), grid, dim3(256), 0, s, a);
  }
}

static void gru_launch_shape(GruGateArgs& a, bool update, int B, hipStream_t s) {
  const bool wide_in = (a.W & 7) == 0 && c3_segments_wide(a.x, B);
  const int shape = c3_pick_shape(a.H, a.W);
  if (shape == 0) gru_launch<4, 64>(a, update, B, wide_in, s);
  else if (shape == 1) gru_launch<8, 32>(a, update, B, wide_in, s);
  else gru_launch<16, 16>(a, update, B, wide_in, s);
}

static C3Segs gru_segments(const void* const* seg, const int64_t* seg_batch_stride, const int* seg_channels, int nseg) {
  C3Segs t = {};
  int first = 0;
  for (int k = 0; k < nseg; k++) {
    t.s[k] = C3Seg{static_cast<const __half*>(seg[k]), seg_batch_stride[k], first, first + seg_channels[k]};
    first += seg_channels[k];
  }
  t.n = nseg;
  return t;
}

static bool gru_wide(const void* p, int64_t batch_stride, int B, int W) {
  return (W & 7) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (B == 1 || (batch_stride & 7) == 0);
}

void launch_gru_gates(const void* const* seg, const int64_t* seg_batch_stride, const int* seg_channels, int nseg,
                      const void* packed, const float* g, void* z, void* rnet, int B, int H, int W, hipStream_t s) {
  GruGateArgs a = {};
  a.x = gru_segments(seg, seg_batch_stride, seg_channels, nseg);
  const int c_in = a.x.s[nseg - 1].end;
  a.wpk = reinterpret_cast<const f16x8*>(gru_parts(packed, c_in).wzr);
  a.g = g;
  a.z = static_cast<__half*>(z);
  a.rnet = static_cast<__half*>(rnet);
  a.net = a.x.s[0].p;
  a.nbs = a.x.s[0].bs;
  a.slabs = c_in / C3_SLAB; a.H = H; a.W = W;
  a.wide_zr = gru_wide(z, 0, 1, W) && gru_wide(rnet, 0, 1, W);   // contiguous: the image stride 128 H W is a multiple of 8
  a.wide_net = gru_wide(a.net, a.nbs, B, W);
  gru_launch_shape(a, false, B, s);
}

void launch_gru_update(const void* const* seg, const int64_t* seg_batch_stride, const int* seg_channels, int nseg,
                       const void* packed, const float* g, const void* z, const void* net, int64_t net_batch_stride,
                       void* out, int64_t out_batch_stride, int B, int H, int W, hipStream_t s) {
  GruGateArgs a = {};
  a.x = gru_segments(seg, seg_batch_stride, seg_channels, nseg);
  const int c_in = a.x.s[nseg - 1].end;
  a.wpk = reinterpret_cast<const f16x8*>(gru_parts(packed, c_in).wq);
  a.g = g;
  a.z = const_cast<__half*>(static_cast<const __half*>(z));
  a.net = static_cast<const __half*>(net);
  a.nbs = net_batch_stride;
  a.out = static_cast<__half*>(out);
  a.obs = out_batch_stride;
  a.slabs = c_in / C3_SLAB; a.H = H; a.W = W;
  a.wide_zr = gru_wide(z, 0, 1, W);
  a.wide_net = gru_wide(net, net_batch_stride, B, W);
  a.wide_out = gru_wide(out, out_batch_stride, B, W);
  gru_launch_shape(a, true, B, s);
}

}  // namespace droid
