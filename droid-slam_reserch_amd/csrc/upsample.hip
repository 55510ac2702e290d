// upsample.hip -- convex upsampling of disparities: `DepthVideo.upsample` (droid_slam/depth_video.py:134-138) with
// `cvx_upsample` (droid_net.py:21-35) behind it, in one launch: the gather disps[ix], the softmax over the 9 taps, the
// 3x3 unfold with zero padding, the weighted sum, the pixel shuffle and the indexed write into disps_up.
// The contract is in include/droid_backends_hip.h (droid_cvx_upsample); byte model and error bar: DESIGN.md.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launchers.hpp"

namespace droid {

__device__ __forceinline__ float cvx_logit(const __half* p) { return __half2float(*p); }   // exact widening
__device__ __forceinline__ float cvx_logit(const float* p) { return *p; }

// Lane mapping: a wave owns 64 consecutive coarse pixels p = y W + x of one frame and ONE sub-pixel row a; the lane of
// pixel p produces the eight sub-pixel columns b of output row 8y + a.
//   mask  [e, c, p], c = k 64 + a 8 + b: for a fixed channel the 64 lanes read 64 consecutive elements (one 128-B / 256-B
//         segment per wave load, every mask byte fetched by exactly one wave, once);
//   out   [f, 8y + a, 8x + b]: a lane writes 32 contiguous bytes, the next lane the next 32 -- 2 KB per wave and row.
// Both sides are coalesced without an LDS transpose.  The 3x3 neighbourhood (9 floats) and the 8 results stay in
// registers; the 72 logits of a lane are streamed, 9 per sub-pixel column.  A workgroup is 4 waves = 4 values of a;
// blockIdx.y picks the half of a, blockIdx.z the batch entry.  No atomics, no LDS, no dependence on n or on the entry's
// position: an output value is a function of its frame's data and its entry's mask alone.
constexpr int CVX_PX = 64;   // coarse pixels per workgroup (one per lane)

template <typename T>
__global__ __launch_bounds__(256) void cvx_upsample_kernel(const float* __restrict__ data, const int64_t* __restrict__ ix,
                                                           const T* __restrict__ mask, float* __restrict__ out,
                                                           int frame0, int nbuf, int H, int W, int vec_store) {
  const int e = blockIdx.z;
  const int64_t f = ix ? ix[e] : (int64_t)frame0 + e;   // compared as the int64 it is
  if (f < 0 || f >= nbuf) return;                       // frame outside both buffers: nothing read, nothing written
  const int HW = H * W;
  const int p = blockIdx.x * CVX_PX + (threadIdx.x & 63);
  if (p >= HW) return;
  const int a = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int y = p / W, x = p - y * W;

  const float* d = data + (size_t)f * HW;
  float P[9];   // F.unfold(., [3,3], padding=1): zero outside the image
#pragma unroll
  for (int ky = 0; ky < 3; ky++)
#pragma unroll
    for (int kx = 0; kx < 3; kx++) {
      const int yy = y + ky - 1, xx = x + kx - 1;
      P[ky * 3 + kx] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? d[(size_t)yy * W + xx] : 0.0f;
    }

  const T* m = mask + ((size_t)e * 576 + a * 8) * HW + p;
  float o[8];
#pragma unroll
  for (int b = 0; b < 8; b++) {
    float l[9];
#pragma unroll
    for (int k = 0; k < 9; k++) l[k] = cvx_logit(m + (size_t)(k * 64 + b) * HW);
    float mx = l[0];
#pragma unroll
    for (int k = 1; k < 9; k++) mx = fmaxf(mx, l[k]);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; k++) {   // max first: |logit| up to 65504 cannot overflow; expf, not a fast intrinsic
      l[k] = expf(l[k] - mx);
      s = (k == 0) ? l[0] : s + l[k];
    }
    float acc = (l[0] / s) * P[0];   // one division per weight, weights stay fp32
#pragma unroll
    for (int k = 1; k < 9; k++) acc = fmaf(l[k] / s, P[k], acc);
    o[b] = acc;
  }

  float* q = out + (size_t)f * 64 * HW + ((size_t)(8 * y + a) * W + x) * 8;
  if (vec_store) {   // the offset is a multiple of 32 bytes: aligned whenever `out` is
    reinterpret_cast<float4*>(q)[0] = make_float4(o[0], o[1], o[2], o[3]);
    reinterpret_cast<float4*>(q)[1] = make_float4(o[4], o[5], o[6], o[7]);
  } else {
#pragma unroll
    for (int b = 0; b < 8; b++) q[b] = o[b];
  }
}

// gridDim.z carries the batch entry and ends at 65535: larger n is launched in slabs, each on the tail of its arrays
// (the convention of launch_projmap, geom.hip).
constexpr int CVX_GRID_Z_MAX = 65535;

void launch_cvx_upsample(const float* data, const int64_t* ix, const void* mask, float* out, int n, int nbuf, int H, int W,
                         bool half_mask, hipStream_t s) {
  const size_t HW = (size_t)H * W;
  const int vec_store = ((uintptr_t)out % 16) == 0;
  const unsigned gx = (unsigned)((HW + CVX_PX - 1) / CVX_PX);
  for (int e0 = 0; e0 < n; e0 += CVX_GRID_Z_MAX) {
    const dim3 grid(gx, 2, min(n - e0, CVX_GRID_Z_MAX));
    const int64_t* ixs = ix ? ix + e0 : nullptr;
    if (half_mask)
      hipLaunchKernelGGL(cvx_upsample_kernel<__half>, grid, dim3(256), 0, s, data, ixs,
                         static_cast<const __half*>(mask) + (size_t)e0 * 576 * HW, out, e0, nbuf, H, W, vec_store);
    else
      hipLaunchKernelGGL(cvx_upsample_kernel<float>, grid, dim3(256), 0, s, data, ixs,
                         static_cast<const float*>(mask) + (size_t)e0 * 576 * HW, out, e0, nbuf, H, W, vec_store);
  }
}

}  // namespace droid
