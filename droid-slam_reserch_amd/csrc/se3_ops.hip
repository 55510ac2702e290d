// se3_ops.hip -- the pose algebra of the inference path: what `PoseTrajectoryFiller.__fill`
// (droid_slam/trajectory_filler.py:43-58), the visualiser, `Droid.terminate` and the multi-session tooling take from
// lietorch -- inv, log, exp, matrix, the group product, and the filler's bracket search + interpolation in one launch.
// The contract (layouts, branch points, the one difference from the reference) is in include/droid_backends_hip.h
// ("pose algebra"); the fp64 helpers are in se3.hpp.  Sixteen poses per chunk: nothing here is a hot path.  One thread
// per record, fp64 from the float32 inputs, one rounding; no LDS, no atomics.  Each thread reads its records before it
// writes, so out may be an input where the header allows it.  Resource figures: DESIGN.md.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/droid_backends_hip.h"
#include "launchers.hpp"
#include "se3.hpp"

namespace droid {

constexpr int SE3_THREADS = 256;
constexpr int SE3_MAX_BLOCKS = 1 << 20;   // more records than that many blocks hold: grid-stride

template <int OP>
__global__ __launch_bounds__(SE3_THREADS) void se3_unary_kernel(const float* in, float* out, int64_t n) {
  const int64_t step = (int64_t)gridDim.x * SE3_THREADS;
  for (int64_t k = (int64_t)blockIdx.x * SE3_THREADS + threadIdx.x; k < n; k += step) {
    if (OP == DROID_SE3_EXP) {
      const float* p = in + 6 * k;
      const double xi[6] = {p[0], p[1], p[2], p[3], p[4], p[5]};
      se3_store(se3_exp_d(xi), out + 7 * k);
    } else {
      const Pose64 a = se3_load(in + 7 * k);
      if (OP == DROID_SE3_INV) {
        se3_store(se3_inv_d(a), out + 7 * k);
      } else if (OP == DROID_SE3_LOG) {
        double xi[6];
        se3_log_d(a, xi);
#pragma unroll
        for (int i = 0; i < 6; i++) out[6 * k + i] = (float)xi[i];
      } else {
        double M[16];
        se3_matrix_d(a, M);
#pragma unroll
        for (int i = 0; i < 16; i++) out[16 * k + i] = (float)M[i];
      }
    }
  }
}

__global__ __launch_bounds__(SE3_THREADS) void se3_mul_kernel(const float* a, int stride_a, const float* b, int stride_b,
                                                              float* out, int64_t n) {
  const int64_t step = (int64_t)gridDim.x * SE3_THREADS;
  for (int64_t k = (int64_t)blockIdx.x * SE3_THREADS + threadIdx.x; k < n; k += step) {
    const Pose64 A = se3_load(a + stride_a * k);
    const Pose64 B = se3_load(b + stride_b * k);
    se3_store(se3_mul_d(A, B), out + 7 * k);
  }
}

// One wave per query.  The wave counts the stamps <= t, 64 per pass (the trip count is wave-uniform, so every lane
// reaches the ballot); lane 0 then does the algebra.  A NaN stamp or a NaN query compares false and is not counted.
__global__ __launch_bounds__(SE3_THREADS) void pose_interpolate_kernel(const float* __restrict__ poses,
                                                                       const float* __restrict__ tstamp, int N,
                                                                       const float* __restrict__ query, int M,
                                                                       float* __restrict__ out, int64_t* __restrict__ k0_out,
                                                                       int64_t* __restrict__ k1_out) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * (SE3_THREADS / 64) + (threadIdx.x >> 6);
  if (m >= M) return;   // a whole wave leaves together
  const float t = query[m];
  int count = 0;
  for (int base = 0; base < N; base += 64) {
    const int k = base + lane;
    const bool hit = k < N && tstamp[k] <= t;
    count += __popcll(__ballot(hit));
  }
  if (lane != 0) return;
  const int k0 = count > 0 ? count - 1 : 0;
  const int k1 = k0 < N - 1 ? k0 + 1 : k0;
  const Pose64 P0 = se3_load(poses + 7 * (int64_t)k0);
  double xi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // k1 == k0: the relative pose is the exact identity
  if (k1 != k0) se3_log_d(se3_mul_d(se3_load(poses + 7 * (int64_t)k1), se3_inv_d(P0)), xi);
  const double ts0 = tstamp[k0];
  const double dt = (double)tstamp[k1] - ts0 + 1e-3;
  const double d = (double)t - ts0;
#pragma unroll
  for (int i = 0; i < 6; i++) xi[i] = xi[i] / dt * d;
  se3_store(se3_mul_d(se3_exp_d(xi), P0), out + 7 * m);
  if (k0_out) k0_out[m] = k0;
  if (k1_out) k1_out[m] = k1;
}

static unsigned se3_blocks(int64_t n) {
  const int64_t b = (n + SE3_THREADS - 1) / SE3_THREADS;
  return (unsigned)(b < SE3_MAX_BLOCKS ? b : SE3_MAX_BLOCKS);
}

void launch_se3_unary(const float* in, float* out, int64_t n, int op, hipStream_t s) {
  const dim3 grid(se3_blocks(n)), block(SE3_THREADS);
  switch (op) {
    case DROID_SE3_INV: hipLaunchKernelGGL(se3_unary_kernel<DROID_SE3_INV>, grid, block, 0, s, in, out, n); break;
    case DROID_SE3_LOG: hipLaunchKernelGGL(se3_unary_kernel<DROID_SE3_LOG>, grid, block, 0, s, in, out, n); break;
    case DROID_SE3_EXP: hipLaunchKernelGGL(se3_unary_kernel<DROID_SE3_EXP>, grid, block, 0, s, in, out, n); break;
    default: hipLaunchKernelGGL(se3_unary_kernel<DROID_SE3_MATRIX>, grid, block, 0, s, in, out, n); break;
  }
}

void launch_se3_mul(const float* a, int stride_a, const float* b, int stride_b, float* out, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(se3_mul_kernel, dim3(se3_blocks(n)), dim3(SE3_THREADS), 0, s, a, stride_a, b, stride_b, out, n);
}

void launch_pose_interpolate(const float* poses, const float* tstamp, int N, const float* query, int M, float* out,
                             int64_t* k0_out, int64_t* k1_out, hipStream_t s) {
  constexpr int per = SE3_THREADS / 64;   // queries per block; M <= 2^31 - 1 gives at most 2^29 blocks
  hipLaunchKernelGGL(pose_interpolate_kernel, dim3((unsigned)(((int64_t)M + per - 1) / per)), dim3(SE3_THREADS), 0, s,
                     poses, tstamp, N, query, M, out, k0_out, k1_out);
}

}  // namespace droid
