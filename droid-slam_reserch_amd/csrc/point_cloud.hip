// point_cloud.hip -- the filtered, coloured point cloud of selected keyframes (visualization.py:100-142 of the
// reference fork and its copies): pose inverse, iproj, depth_filter, the count / disparity rule, the colour lookup and
// the ordered compaction in three launches on the caller's stream.  The contract is in include/droid_backends_hip.h
// (droid_point_cloud); launch structure and resource figures: DESIGN.md.
//
//   1. pc_decide   one workgroup per (selection, 256-pixel tile): the frame mean in fp64 (every tile re-reads its frame,
//                  12 KB at 48 x 64, from L2, all in the same order, so all tiles of a frame hold the same bits), the
//                  depth_filter count, the keep rule, one ballot per wave.  Writes four 64-bit keep words and one count
//                  per tile -- for every tile, invalid selections included, so nothing depends on what the workspace held.
//   2. pc_scan     ONE workgroup: exclusive scan of the tile counts in place (4096 per pass), offsets[b] where a
//                  selection starts, offsets[n] at the end.
//   3. pc_emit     the grid of launch 1: rank of a lane inside its wave's keep word (popcount of the lower lanes), plus the
//                  popcounts of the earlier waves of the tile, plus the tile's base: the final row.  Point, colour and
//                  src are written there; the first tile of a selection writes its matrix.
// No atomics and no workgroup waits for another: the order of the rows is the order of (selection, pixel) by
// construction, and the stream orders the launches.  Rows at and beyond offsets[n] are never written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/droid_backends_hip.h"
#include "launchers.hpp"
#include "se3.hpp"

namespace droid {

constexpr int PC_THREADS = 256;             // one tile: 4 waves
constexpr int PC_WAVES = PC_THREADS / 64;
constexpr int PC_SCAN_THREADS = 1024;
constexpr int PC_SCAN_ITEMS = 4;            // tile counts per thread and pass
constexpr int PC_GRID_MAX = 65536;          // tiles per launch of the two pixel grids

__device__ __forceinline__ double wave_sum_d(double s) {
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  return s;
}

__global__ __launch_bounds__(PC_THREADS) void pc_decide_kernel(
    const float* __restrict__ poses, const float* __restrict__ disps, const float* __restrict__ intrinsics,
    const int64_t* __restrict__ index, const float* __restrict__ thresh, unsigned long long* __restrict__ words,
    int* __restrict__ tiles, unsigned first, int nbuf, int H, int W, int nt, int min_count, double disp_ratio) {
  __shared__ double part[PC_WAVES];
  __shared__ int pop[PC_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned gt = first + blockIdx.x;   // tile of the call: selection * nt + tile of the frame
  const int b = gt / nt, tile = gt - b * nt;
  const int HW = H * W;
  const int64_t i64 = index[b];   // tested before it is narrowed: 2^32 + 3 is not frame 3
  const bool live = i64 >= 0 && i64 < nbuf;
  bool keep = false;
  if (live) {   // uniform over the workgroup
    const int ix = (int)i64;
    const float* dp = disps + (size_t)ix * HW;
    double s = 0.0;
    for (int k = tid; k < HW; k += PC_THREADS) s += (double)dp[k];
    s = wave_sum_d(s);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    const double mean = (part[0] + part[1] + part[2] + part[3]) / (double)HW;
    const int k = tile * PC_THREADS + tid;
    if (k < HW) {
      const Intr K = {intrinsics[0], intrinsics[1], intrinsics[2], intrinsics[3]};
      const float cnt = depth_filter_count(poses, disps, K, ix, thresh[b], k, nbuf, H, W);
      keep = (int)cnt >= min_count && (double)dp[k] > disp_ratio * mean;
    }
  }
  const unsigned long long word = __ballot(keep);
  if (lane == 0) {
    words[(size_t)gt * PC_WAVES + wave] = word;
    pop[wave] = __popcll(word);
  }
  __syncthreads();
  if (tid == 0) tiles[gt] = pop[0] + pop[1] + pop[2] + pop[3];
}

// tiles [T]: counts in, exclusive prefix sums out.  The total stays below 2^31 (n * h * w does).
__global__ __launch_bounds__(PC_SCAN_THREADS) void pc_scan_kernel(int* __restrict__ tiles, int* __restrict__ offsets,
                                                                  unsigned T, unsigned nt, int n) {
  __shared__ int wsum[PC_SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  // T < 2^31, so a tile number plus one pass (4096) stays inside 32 bits
  for (unsigned base = 0; base < T; base += PC_SCAN_THREADS * PC_SCAN_ITEMS) {
    const unsigned j0 = base + tid * PC_SCAN_ITEMS;
    int c[PC_SCAN_ITEMS];
    int s = 0;
#pragma unroll
    for (int m = 0; m < PC_SCAN_ITEMS; m++) {
      c[m] = j0 + m < T ? tiles[j0 + m] : 0;
      s += c[m];
    }
    int incl = s;   // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int v = __shfl_up(incl, off);
      if (lane >= off) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < PC_SCAN_THREADS / 64; w++) {
      const int v = wsum[w];
      if (w < wave) before += v;
      all += v;
    }
    int run = carry + before + incl - s;
#pragma unroll
    for (int m = 0; m < PC_SCAN_ITEMS; m++) {
      const unsigned j = j0 + m;
      if (j < T) {
        tiles[j] = run;
        if (j % nt == 0) offsets[j / nt] = run;   // the first tile of a selection
        run += c[m];
      }
    }
    carry += all;
    __syncthreads();   // wsum is rewritten by the next pass
  }
  if (tid == 0) offsets[n] = carry;
}

__global__ __launch_bounds__(PC_THREADS) void pc_emit_kernel(
    const float* __restrict__ poses, const float* __restrict__ disps, const float* __restrict__ intrinsics,
    const int64_t* __restrict__ index, const uint8_t* __restrict__ images, const unsigned long long* __restrict__ words,
    const int* __restrict__ tiles, float* __restrict__ points, float* __restrict__ colors, int* __restrict__ src,
    float* __restrict__ matrices, unsigned first, int nbuf, int H, int W, int nt) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned gt = first + blockIdx.x;
  const int b = gt / nt, tile = gt - b * nt;
  const int64_t i64 = index[b];
  if (i64 < 0 || i64 >= nbuf) {   // no rows; the matrix is all zero
    if (tile == 0 && tid < 16) matrices[(size_t)b * 16 + tid] = 0.f;
    return;
  }
  const int ix = (int)i64;
  const Pose64 G = se3_inv_d(se3_load(poses + 7 * (size_t)ix));
  if (tile == 0 && tid == 0) {
    double M[16];
    se3_matrix_d(G, M);
#pragma unroll
    for (int m = 0; m < 16; m++) matrices[(size_t)b * 16 + m] = (float)M[m];
  }
  const unsigned long long* tw = words + (size_t)gt * PC_WAVES;
  const unsigned long long word = tw[wave];
  if (!((word >> lane) & 1ull)) return;
  int row = tiles[gt];
#pragma unroll
  for (int w = 0; w < PC_WAVES - 1; w++)
    if (w < wave) row += __popcll(tw[w]);
  row += __popcll(word & ((1ull << lane) - 1ull));
  const int HW = H * W;
  const int k = tile * PC_THREADS + tid;   // < HW: pc_decide keeps nothing beyond the frame
  const int u = k % W, v = k / W;
  const double fx = intrinsics[0], fy = intrinsics[1], cx = intrinsics[2], cy = intrinsics[3];
  const double r = 1.0 / (double)disps[(size_t)ix * HW + k];
  const double X[3] = {((double)u - cx) / fx * r, ((double)v - cy) / fy * r, r};
  double Y[3];
  act_so3_d(G.q, X, Y);
  float* p = points + (size_t)row * 3;
  p[0] = (float)(Y[0] + G.t[0]);
  p[1] = (float)(Y[1] + G.t[1]);
  p[2] = (float)(Y[2] + G.t[2]);
  src[row] = k;
  if (images) {
    const size_t plane = (size_t)64 * HW, pitch = (size_t)8 * W;
    const uint8_t* px = images + (size_t)ix * 3 * plane + (size_t)(8 * v + 3) * pitch + (8 * u + 3);
    float* c = colors + (size_t)row * 3;
    c[0] = __fdiv_rn((float)px[2 * plane], 255.0f);   // stored BGR, returned RGB
    c[1] = __fdiv_rn((float)px[plane], 255.0f);
    c[2] = __fdiv_rn((float)px[0], 255.0f);
  }
}

static int64_t pc_tiles_per_frame(int H, int W) { return ((int64_t)H * W + PC_THREADS - 1) / PC_THREADS; }

// keep words [T * 4] uint64, then tile counts / bases [T] int32, T = n * ceil(h w / 256)
size_t point_cloud_workspace_bytes(int n, int H, int W) {
  return (size_t)n * (size_t)pc_tiles_per_frame(H, W) * (PC_WAVES * sizeof(unsigned long long) + sizeof(int));
}

void launch_point_cloud(const float* poses, const float* disps, const float* intr, const int64_t* index,
                        const float* thresh, const uint8_t* images, int n, int nbuf, int H, int W, int min_count,
                        double disp_ratio, float* points, float* colors, int* src, int* offsets, float* matrices,
                        void* workspace, hipStream_t s) {
  const int nt = (int)pc_tiles_per_frame(H, W);
  const int64_t T = (int64_t)n * nt;   // <= n * h * w < 2^31
  unsigned long long* words = (unsigned long long*)workspace;
  int* tiles = (int*)(words + T * PC_WAVES);
  // (selection, tile) lies on grid.x; beyond PC_GRID_MAX tiles (16.7 M pixels) the two grids go out in slabs
  for (int64_t t0 = 0; t0 < T; t0 += PC_GRID_MAX)
    hipLaunchKernelGGL(pc_decide_kernel, dim3((unsigned)(T - t0 < PC_GRID_MAX ? T - t0 : PC_GRID_MAX)), dim3(PC_THREADS), 0,
                       s, poses, disps, intr, index, thresh, words, tiles, (unsigned)t0, nbuf, H, W, nt, min_count,
                       disp_ratio);
  hipLaunchKernelGGL(pc_scan_kernel, dim3(1), dim3(PC_SCAN_THREADS), 0, s, tiles, offsets, (unsigned)T, (unsigned)nt, n);
  for (int64_t t0 = 0; t0 < T; t0 += PC_GRID_MAX)
    hipLaunchKernelGGL(pc_emit_kernel, dim3((unsigned)(T - t0 < PC_GRID_MAX ? T - t0 : PC_GRID_MAX)), dim3(PC_THREADS), 0,
                       s, poses, disps, intr, index, images, words, tiles, points, colors, src, matrices, (unsigned)t0, nbuf,
                       H, W, nt);
}

}  // namespace droid
