// graph.hpp -- host-side view of the proximity-edge selection (graph.hip), shared with api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace droid {

constexpr int PROX_MAX_CELLS = 1 << 20;   // suppression bitmap of the rectangle: 128 KB of the CU's 160 KB LDS
constexpr int PROX_CHUNK = 16384;         // candidates one workgroup sorts in LDS (128 KB of 8-byte keys)

struct ProxArgs {
  const float* dist;   // directed frame distances, dist[i * ld + j] for the edge i -> j
  int ld, bidir;
  int t, t0, t1, rad, nms;
  float thresh;
  int max_factors, stereo;
  const int64_t *sup_ii, *sup_jj;
  int n_sup;
  const int64_t *known_ii, *known_jj;
  int n_known;
  int64_t* out;        // [cap, 2]
  int cap;
  int* count_out;
  void* ws;
};

// edges step 4 of the contract always emits: rows i in [t0, t), (i, i) when stereo, then (i, j), (j, i) for the
// min(i, rad + 1) frames before i
__host__ __device__ inline int64_t prox_forced_before(int64_t i, int64_t m) {   // sum over k < i of min(k, m)
  return i <= m + 1 ? i * (i - 1) / 2 : m * (m + 1) / 2 + (i - 1 - m) * m;
}
__host__ __device__ inline int64_t prox_forced_edges(int t, int t0, int rad, int stereo) {
  if (t <= t0) return 0;
  return (stereo ? (int64_t)(t - t0) : 0) + 2 * (prox_forced_before(t, (int64_t)rad + 1) - prox_forced_before(t0, (int64_t)rad + 1));
}
// most edges a call can produce before the known-edge filter
inline int64_t prox_edge_bound(int t, int t0, int t1, int rad, int max_factors, int stereo) {
  if (t <= t0) return 0;
  const int64_t forced = prox_forced_edges(t, t0, rad, stereo);
  const int64_t all = forced + 2 * (int64_t)(t - t0) * (t - t1);
  const int64_t walk = (int64_t)max_factors + 2 < all ? (int64_t)max_factors + 2 : all;
  return forced > walk ? forced : walk;
}

size_t prox_workspace_bytes(int t, int t0, int t1, int n_known, int cap);
void launch_proximity_edges(const ProxArgs& a, hipStream_t s);

}  // namespace droid
