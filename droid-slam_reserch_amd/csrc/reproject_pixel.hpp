// reproject_pixel.hpp -- the per-edge setup and the per-pixel body of reproject + motion features, shared by
// reproject_motion_kernel (geom.hip) and motion_encode_kernel (motion_encode.hip) so that both produce the same bits:
//   depth_video.py:150-158 `reproject` -> geom/projective_ops.py:96-125 `projective_transform`
//   (back-projection with the SOURCE frame's intrinsics :99, Gij = Gj * Gi^-1 :102, stereo edges ii == jj use
//   the fixed baseline (-0.1, 0, 0) :105, projection with the TARGET frame's intrinsics where a depth below
//   0.5 * MIN_DEPTH is replaced by 1 :46-51, valid = depth > MIN_DEPTH = 0.2 :113 -- these are the Python-side
//   constants, not the 0.25 of droid_kernels.cu), then factor_graph.py:203-205:
//   motn = clamp(cat(coords1 - coords0, target - coords1), -64, 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "se3.hpp"

namespace droid {

struct ReprojEdge {
  Intr Ki;      // source frame
  float kj[4];  // target frame
  Rel T;
};

// i64, j64 lie inside the buffer (the caller has compared them as the int64 they are)
__device__ __forceinline__ ReprojEdge reproject_edge(const float* __restrict__ poses, const float* __restrict__ intrinsics,
                                                     int intr_stride, int64_t i64, int64_t j64) {
  const float* ki = intrinsics + (size_t)i64 * intr_stride;
  const float* kj = intrinsics + (size_t)j64 * intr_stride;
  ReprojEdge g;
  g.Ki = {ki[0], ki[1], ki[2], ki[3]};
  g.kj[0] = kj[0]; g.kj[1] = kj[1]; g.kj[2] = kj[2]; g.kj[3] = kj[3];
  g.T = rel_pose<true>(poses, (int)i64, (int)j64);
  return g;
}

// pixel (u, v) with disparity `disp` of the source frame: coordinates in the target frame and the validity flag.
// transform_pixel (se3.hpp: back-projection, act_so3, + disp * t) and the projection with EVERY rounding written out:
// under the default -ffp-contract=fast the compiler chooses which product of a sum it fuses from the code around the
// call, and the two kernels that share this function have to give the same bits.  The choices below are the ones the
// compiler made for reproject_motion_kernel while the expression was left to it, so that operator's bits are the ones
// it always had: where act_so3's uv terms feed a sum they are the fused forms (uv0, uv1, uv2a, uv2b -- the two forms of
// uv2 differ in which product is rounded), where they feed a product of the last row the unfused ones (uv0r, uv1r).
// This DELIBERATELY duplicates transform_pixel / act_so3 of se3.hpp (with X2 = 1) instead of calling them: a change to
// the arithmetic there has to be mirrored here.  tests/test_gpu_reproject_bits.py holds the operator to recorded bits.
__device__ __forceinline__ float2 reproject_pixel(const ReprojEdge& g, float u, float v, float disp, float& valid) {
#pragma clang fp contract(off)
  const float q0 = g.T.q[0], q1 = g.T.q[1], q2 = g.T.q[2], q3 = g.T.q[3];
  const float X0 = (u - g.Ki.cx) / g.Ki.fx, X1 = (v - g.Ki.cy) / g.Ki.fy;   // X2 = 1
  const float uv0 = 2.0f * __builtin_fmaf(-q2, X1, q1), uv0r = 2.0f * (q1 - q2 * X1);
  const float uv1 = 2.0f * __builtin_fmaf(q2, X0, -q0), uv1r = 2.0f * (q2 * X0 - q0);
  const float uv2a = 2.0f * __builtin_fmaf(-q1, X0, q0 * X1), uv2b = 2.0f * __builtin_fmaf(q0, X1, -(q1 * X0));
  const float Y0 = __builtin_fmaf(q3, uv0r, X0) + __builtin_fmaf(q1, uv2a, -(q2 * uv1));
  const float Y1 = __builtin_fmaf(q3, uv1r, X1) + __builtin_fmaf(q2, uv0, -(q0 * uv2b));
  const float Y2 = __builtin_fmaf(q3, uv2a, 1.0f) + (q0 * uv1r - q1 * uv0r);
  const float Xj0 = __builtin_fmaf(g.T.t[0], disp, Y0), Xj1 = __builtin_fmaf(g.T.t[1], disp, Y1);
  const float Z = __builtin_fmaf(g.T.t[2], disp, Y2);
  const float d = 1.0f / ((Z < 0.5f * 0.2f) ? 1.0f : Z);
  const float x = __builtin_fmaf(g.kj[0], Xj0 * d, g.kj[2]);
  const float y = __builtin_fmaf(g.kj[1], Xj1 * d, g.kj[3]);
  valid = (Z > 0.2f) ? 1.0f : 0.0f;  // the source point has depth 1 > MIN_DEPTH by construction
  return make_float2(x, y);
}

// the four motion planes of the pixel: always finite and within +-64 (fminf / fmaxf drop a NaN)
__device__ __forceinline__ void motion_pixel(float2 xy, float u, float v, float2 tg, float (&m)[4]) {
#pragma clang fp contract(off)
  auto clamp64 = [](float a) { return fminf(fmaxf(a, -64.0f), 64.0f); };
  m[0] = clamp64(xy.x - u);
  m[1] = clamp64(xy.y - v);
  m[2] = clamp64(tg.x - xy.x);
  m[3] = clamp64(tg.y - xy.y);
}

}  // namespace droid
