// motion_encode.hip -- reproject + motion features fused with flow_encoder[0:2] of the update module, a
// Conv2d(4, 128, 7, padding=3) and a ReLU under autocast (include/droid_motion_encode_hip.h).
//
// One wave per workgroup owns 64 consecutive pixels of one edge, as in corr_encode_kernel (encode_tile.hpp: the A tile,
// the MFMA loop and the epilogue are that kernel's).  The convolution is the GEMM K = 4 x 49 against 128 channels with
// the motion channel standing where the pyramid level stands.
//   1. Patch.  The wave evaluates the motion features of every pixel the 7 x 7 windows of its 64 pixels touch -- image
//      rows v_min - 3 .. v_max + 3 -- with reproject_pixel.hpp, the arithmetic of reproject_motion_kernel, and keeps
//      half(m) per channel in LDS; positions outside the image are written as zeros.  The interior pixels' coords /
//      valid are stored from the same evaluation.  The columns of the patch are a cyclic window of the padded row
//      (period P = W + 6, MP_COLS columns at most): a wave whose pixels wrap from the end of one row to the start of
//      the next needs the last columns of the row and the first ones, which are neighbours on the cycle, so the patch
//      stays bounded whatever W is (mp_positions_max).
//   2. Per channel every lane copies the 49 halves of its pixel's window into its row of the A tile and the tile meets
//      the channel's packed weights in ce_mma; the accumulators live across the four channels.
// Every LDS byte the MFMA operands read is written by this launch: the patch positions a window reads, the 49 columns
// of every tile row (lanes without a pixel write zeros) and the padding columns 49 .. 63.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/droid_motion_encode_hip.h"
#include "encode_tile.hpp"
#include "launchers.hpp"
#include "reproject_pixel.hpp"

namespace droid {

constexpr int MP_COLS = 76;  // 64 pixels + 6 halo columns on each side of a wrap
// positions of the patch at width W: (rows the 64 pixels can span + 6) x min(W + 6, MP_COLS)
constexpr int mp_positions(int W) { return (2 + 62 / W + 6) * (W + 6 < MP_COLS ? W + 6 : MP_COLS); }
constexpr int mp_positions_max() {
  int m = 0;
  for (int W = 1; W <= 128; W++) m = mp_positions(W) > m ? mp_positions(W) : m;  // constant from W = 70 on
  return m;
}
constexpr int MP_MAX = 640;
static_assert(mp_positions_max() <= MP_MAX && mp_positions(1 << 30) <= MP_MAX, "the LDS patch holds every shape");

struct MotionEncodeArgs {
  const float *poses, *disps, *intrinsics;
  int intr_stride;
  const int64_t *ii, *jj;
  const float *target, *motn_in;
  const f16x8* wpk;
  const __half* b16;
  float *coords, *valid;
  __half* y;
  int nbuf, H, W;
};

// GIVEN: m is read from motn_in [E,4,H,W]; else it is evaluated from the geometry and coords / valid are written
template <bool GIVEN>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void motion_encode_kernel(const MotionEncodeArgs a) {
  __shared__ __attribute__((aligned(16))) _Float16 tile[64 * CE_PITCH];
  __shared__ _Float16 patch[4][MP_MAX];
  const int lane = threadIdx.x, H = a.H, W = a.W, HW = H * W;
  const int pix0 = blockIdx.x * 64, e = blockIdx.y;
  const int last = min(pix0 + 63, HW - 1);
  const int v_min = pix0 / W, v_max = last / W;
  const int P = W + 6;                         // the padded row, column c at cyclic position c + 3
  const int NC = min(P, MP_COLS), NR = v_max - v_min + 7;
  const int s0 = P <= MP_COLS ? 0 : pix0 - v_min * W;   // cyclic position of the patch's first column
  _Float16* row = tile + lane * CE_PITCH;
  {  // the padding columns: zeros of the kernel's own, whatever the LDS held (column 48 is rewritten by every channel)
    const uint4 z = {0u, 0u, 0u, 0u};
    *reinterpret_cast<uint4*>(row + 48) = z;
    *reinterpret_cast<uint4*>(row + 56) = z;
  }
  // ---- 1. the patch
  bool live = true;
  int64_t i64 = 0;
  ReprojEdge g;
  if constexpr (!GIVEN) {
    i64 = a.ii[e];
    const int64_t j64 = a.jj[e];
    live = !(i64 < 0 || i64 >= a.nbuf || j64 < 0 || j64 >= a.nbuf);  // edge with a bad index: m = 0, zeros, no fault
    if (live) g = reproject_edge(a.poses, a.intrinsics, a.intr_stride, i64, j64);
  }
  for (int idx = lane; idx < NR * NC; idx += 64) {
    const int pr = idx / NC, pc = idx - pr * NC;
    const int r = v_min - 3 + pr;
    int cyc = s0 + pc;
    if (cyc >= P) cyc -= P;
    const int c = cyc - 3;
    float m[4] = {0.f, 0.f, 0.f, 0.f};
    if (r >= 0 && r < H && c >= 0 && c < W) {
      const int k = r * W + c;
      if constexpr (GIVEN) {
        const float* src = a.motn_in + (size_t)e * 4 * HW + k;
#pragma unroll
        for (int ch = 0; ch < 4; ch++) m[ch] = src[(size_t)ch * HW];
      } else {
        const size_t o = (size_t)e * HW + k;
        const bool own = k >= pix0 && k < pix0 + 64;   // every pixel of the image is owned by one wave
        if (live) {
          const float u = (float)c, v = (float)r;
          float vl;
          const float2 xy = reproject_pixel(g, u, v, a.disps[(size_t)i64 * HW + k], vl);
          motion_pixel(xy, u, v, reinterpret_cast<const float2*>(a.target)[o], m);
          if (own) {
            reinterpret_cast<float2*>(a.coords)[o] = xy;
            a.valid[o] = vl;
          }
        } else if (own) {
          reinterpret_cast<float2*>(a.coords)[o] = make_float2(0.f, 0.f);
          a.valid[o] = 0.f;
        }
      }
    }
#pragma unroll
    for (int ch = 0; ch < 4; ch++) {  // autocast's cast in front of the convolution: nearest-even (|m| <= 64: no overflow)
      const __half h = __float2half_rn(m[ch]);
      patch[ch][idx] = __builtin_bit_cast(_Float16, h);
    }
  }
  // ---- 2. the four channels
  const bool has_pixel = pix0 + lane < HW;
  const int pix = has_pixel ? pix0 + lane : HW - 1;
  const int pv = pix / W, pu = pix - pv * W;
  int pcb = pu - s0;               // patch column of tap kx = 0 (image column pu - 3)
  if (pcb < 0) pcb += P;
  const int base = (pv - v_min) * NC + pcb;   // tap (ky, kx) is at base + ky * NC + kx
  const int gq = lane >> 4, c16 = lane & 15, arow = ce_arow(c16);
  f32x4 acc[8][4];  // [channel tile][pixel tile]
#pragma unroll
  for (int nt = 0; nt < 8; nt++)
#pragma unroll
    for (int t = 0; t < 4; t++) acc[nt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();  // the patch is complete
#pragma unroll 1
  for (int ch = 0; ch < 4; ch++) {
    const _Float16* src = patch[ch] + base;
    f16x8 w8[6];
    _Float16 w48 = (_Float16)0.f;
#pragma unroll
    for (int k = 0; k < 48; k++) w8[k >> 3][k & 7] = has_pixel ? src[(k / 7) * NC + (k % 7)] : (_Float16)0.f;
    if (has_pixel) w48 = src[6 * NC + 6];
    if (ch > 0) __syncthreads();  // the previous channel's fragments have been read
#pragma unroll
    for (int q = 0; q < 6; q++) *reinterpret_cast<f16x8*>(row + 8 * q) = w8[q];
    row[48] = w48;
    __syncthreads();
    ce_mma(tile, a.wpk, ch, lane, gq, arow, acc);
  }
  const int p0 = pix0 + 16 * gq;
  const bool wide = (HW & 7) == 0 && (reinterpret_cast<uintptr_t>(a.y) & 15) == 0 && p0 + 16 <= HW;
#pragma unroll
  for (int nt = 0; nt < 8; nt++) ce_store(acc[nt], nt * 16 + c16, a.b16, a.y, e, HW, p0, wide);
}

// every argument has been checked by droid_motion_encode
void launch_motion_encode(const float* poses, const float* disps, const float* intr, int intr_stride, const int64_t* ii,
                          const int64_t* jj, const float* target, const float* motn_in, const void* packed, float* coords,
                          float* valid, void* out, int E, int nbuf, int H, int W, hipStream_t s) {
  static_assert(DROID_CORR_ENCODE_PACKED_BYTES == (CE_LEVELS * CE_KP * CE_N + CE_N) * 2, "one packed layout for both encoders");
  MotionEncodeArgs a;
  a.poses = poses; a.disps = disps; a.intrinsics = intr; a.intr_stride = intr_stride;
  a.ii = ii; a.jj = jj; a.target = target; a.motn_in = motn_in;
  a.wpk = static_cast<const f16x8*>(packed);
  a.b16 = static_cast<const __half*>(packed) + (size_t)CE_LEVELS * CE_KP * CE_N;
  a.coords = coords; a.valid = valid;
  a.y = static_cast<__half*>(out);
  a.nbuf = nbuf; a.H = H; a.W = W;
  const dim3 grid((H * W + 63) / 64, E);
  if (motn_in) hipLaunchKernelGGL(motion_encode_kernel<true>, grid, dim3(64), 0, s, a);
  else hipLaunchKernelGGL(motion_encode_kernel<false>, grid, dim3(64), 0, s, a);
}

}  // namespace droid
