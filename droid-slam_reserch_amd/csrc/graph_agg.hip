// graph_agg.hip -- the source-frame mean of the update operator: `GraphAgg.forward` (droid_slam/droid_net.py:59-75),
//   _, ix = torch.unique(ii, return_inverse=True);  net = scatter_mean(net.view(batch, num, 128, ht, wd), ix, dim=1)
// as two launches on one stream: a one-workgroup prepare that turns the index into per-group entry lists, and a reduce
// that streams every row of src once and writes every row of out once.  The contract (grouping, arithmetic, limits) is
// in include/droid_backends_hip.h (droid_graph_mean); error bound, resource figures and why the additions stay
// sequential: DESIGN.md.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/droid_backends_hip.h"
#include "launchers.hpp"

namespace droid {

// ------------------------------------------------------------------------------------------------------------- prepare
// One workgroup of 1024 threads.  LDS tables over the values [0, range):
//   cnt16[v]  entries with index == v, then (in place) the offset of v's list in `entries`.  E <= 65535, so a count and
//             an offset both fit 16 bits; counting adds 1 << 16 (v & 1) to the 32-bit word that holds two of them, and
//             since all counts together are at most 65535 the low half never carries into the high one.
//   bits[w]   presence bitmap, 32 values per word;   wrank[w]  set bits in the words before w (compact mode: the rank
//             of a value among the distinct ones is wrank[v >> 5] + popcount of the lower bits of its word).
// Workspace: offsets [range + 1] int32 (row g owns entries[offsets[g] .. offsets[g + 1])), then entries [E] int32.
// Rows from the distinct count onward (compact mode) get the number of in-range entries as their offset: empty.
constexpr int GM_PREP_THREADS = 1024;
constexpr int GM_WORDS = DROID_GRAPH_MEAN_MAX_RANGE / 32;
constexpr int GM_SCAN = 16;   // entries of `index` fetched per step of the list walk
constexpr int GM_SORT_MAX = DROID_GRAPH_MEAN_MAX_RANGE / 2;   // keys the count table's words hold once it is consumed

// exclusive prefix of one int per thread over the workgroup (every thread calls it); *total = the sum
__device__ __forceinline__ int block_exclusive_scan(int x, int* wave_sums /*[16] LDS*/, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(inc, d, 64);
    if (lane >= d) inc += y;
  }
  __syncthreads();   // wave_sums may still be read from an earlier scan
  if (lane == 63) wave_sums[wave] = inc;
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < GM_PREP_THREADS / 64; w++) {
    const int s = wave_sums[w];
    if (w < wave) base += s;
    sum += s;
  }
  *total = sum;
  return base + inc - x;
}

__global__ __launch_bounds__(GM_PREP_THREADS) void graph_mean_prepare_kernel(const int64_t* __restrict__ index, int E,
                                                                             int range, int compact,
                                                                             int* __restrict__ offsets,
                                                                             int* __restrict__ entries,
                                                                             int* __restrict__ groups_out) {
  __shared__ uint32_t cnt32[DROID_GRAPH_MEAN_MAX_RANGE / 2];
  __shared__ uint32_t bits[GM_WORDS];
  __shared__ int wrank[GM_WORDS];
  __shared__ int wave_sums[GM_PREP_THREADS / 64];
  uint16_t* cnt16 = reinterpret_cast<uint16_t*>(cnt32);
  const int t = threadIdx.x;
  const int nwords = (range + 31) >> 5;

  for (int i = t; i < (range + 1) / 2; i += GM_PREP_THREADS) cnt32[i] = 0;
  for (int i = t; i < nwords; i += GM_PREP_THREADS) bits[i] = 0;
  __syncthreads();
  for (int e = t; e < E; e += GM_PREP_THREADS) {
    const int64_t v = index[e];   // compared as the int64 it is: 2^40 is no frame
    if (v >= 0 && v < range) {
      atomicAdd(&cnt32[v >> 1], 1u << (16 * ((int)v & 1)));
      atomicOr(&bits[v >> 5], 1u << ((int)v & 31));
    }
  }
  __syncthreads();

  // rank of every bitmap word (GM_WORDS <= the workgroup: one word per thread)
  int ngroups;
  {
    const int pc = t < nwords ? __popc(bits[t]) : 0;
    const int ex = block_exclusive_scan(pc, wave_sums, &ngroups);
    if (t < nwords) wrank[t] = ex;
  }
  // offsets of the lists: thread t owns the values [t per, (t + 1) per)
  const int per = (range + GM_PREP_THREADS - 1) / GM_PREP_THREADS;
  const int v0 = min(t * per, range), v1 = min(v0 + per, range);
  int mine = 0;
  for (int v = v0; v < v1; v++) mine += cnt16[v];
  int in_range;
  int run = block_exclusive_scan(mine, wave_sums, &in_range);   // its barriers also publish wrank
  for (int v = v0; v < v1; v++) {
    const int c = cnt16[v];
    cnt16[v] = (uint16_t)run;   // a 16-bit store: the neighbour in the same word belongs to another thread
    const uint32_t w = bits[v >> 5];
    if (!compact)
      offsets[v] = run;
    else if ((w >> (v & 31)) & 1u)
      offsets[wrank[v >> 5] + __popc(w & ((1u << (v & 31)) - 1u))] = run;
    run += c;
  }
  if (compact)
    for (int g = ngroups + t; g <= range; g += GM_PREP_THREADS) offsets[g] = in_range;
  else if (t == 0)
    offsets[range] = in_range;
  if (t == 0 && groups_out) *groups_out = ngroups;
  __syncthreads();

  // the lists, in ascending e.  Up to GM_SORT_MAX entries: the keys (value << 16 | e) -- pairwise distinct, an ignored
  // entry all ones -- are sorted in LDS (bitonic, in the words the counts have just vacated); their order is every
  // list in turn, each in ascending e.
  if (E <= GM_SORT_MAX) {
    uint32_t* keys = cnt32;
    int n = 1;
    while (n < E) n <<= 1;
    for (int i = t; i < n; i += GM_PREP_THREADS) {
      uint32_t key = 0xFFFFFFFFu;
      if (i < E) {
        const int64_t v = index[i];
        if (v >= 0 && v < range) key = ((uint32_t)v << 16) | (uint32_t)i;
      }
      keys[i] = key;
    }
    for (int k = 2; k <= n; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        __syncthreads();
        for (int i = t; i < (n >> 1); i += GM_PREP_THREADS) {
          const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
          const uint32_t x = keys[lo], y = keys[hi];
          if ((x > y) == ((lo & k) == 0)) {
            keys[lo] = y;
            keys[hi] = x;
          }
        }
      }
    __syncthreads();
    for (int i = t; i < in_range; i += GM_PREP_THREADS) entries[i] = (int)(keys[i] & 0xFFFFu);
    return;
  }
  // Longer lists: one thread per value walks the whole index (a wave-uniform address: scalar loads, GM_SCAN in flight)
  // and keeps the entries that are its own.  A wave none of whose 64 values is present has nothing to do.
  for (int vb = (t & ~63); vb < range; vb += GM_PREP_THREADS) {
    const int v = vb + (t & 63);
    const bool present = v < range && ((bits[v >> 5] >> (v & 31)) & 1u);
    if (!__any(present)) continue;
    int pos = present ? cnt16[v] : E;   // pos < E holds for a present value unless index changed under us
    const int64_t want = v;
    int e = 0;
    for (; e + GM_SCAN <= E; e += GM_SCAN) {
      int64_t x[GM_SCAN];
#pragma unroll
      for (int u = 0; u < GM_SCAN; u++) x[u] = index[e + u];
#pragma unroll
      for (int u = 0; u < GM_SCAN; u++)
        if (x[u] == want && pos < E) entries[pos++] = e + u;
    }
    for (; e < E; e++)
      if (index[e] == want && pos < E) entries[pos++] = e;
  }
}

// -------------------------------------------------------------------------------------------------------------- reduce
// grid (tiles of the plane, rows of out); a thread owns 16 bytes of the row.  The entry list of the row is wave-uniform
// (scalar loads); GM_UNROLL rows are loaded before the first of them is added, and the additions run strictly in list
// order.  VEC: src and out 16-byte aligned and the row pitch a multiple of 16 bytes -- one 16-byte load per entry and one
// 16-byte store.  Otherwise the same thread handles the same elements one by one (bounds-checked): the arithmetic per
// element is the same, so are the bits.  No LDS, no atomics.
constexpr int GM_THREADS = 256;
constexpr int GM_UNROLL = 4;

template <typename T> struct GmChunk;
template <> struct GmChunk<__half> { static constexpr int N = 8; };
template <> struct GmChunk<float> { static constexpr int N = 4; };

__device__ __forceinline__ float gm_widen(__half x) { return __half2float(x); }   // exact, subnormals kept
__device__ __forceinline__ float gm_widen(float x) { return x; }
__device__ __forceinline__ void gm_narrow(float q, __half* p) { *p = __float2half_rn(q); }
__device__ __forceinline__ void gm_narrow(float q, float* p) { *p = q; }

template <typename T, bool VEC>
__device__ __forceinline__ void gm_load(const T* __restrict__ p, int valid, float (&x)[GmChunk<T>::N]) {
  constexpr int N = GmChunk<T>::N;
  if (VEC) {
    const uint4 raw = *reinterpret_cast<const uint4*>(p);
    const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
    for (int i = 0; i < N; i++) x[i] = gm_widen(e[i]);
  } else {
#pragma unroll
    for (int i = 0; i < N; i++) x[i] = i < valid ? gm_widen(p[i]) : 0.0f;
  }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(GM_THREADS) void graph_mean_reduce_kernel(const T* __restrict__ src,
                                                                       const int* __restrict__ offsets,
                                                                       const int* __restrict__ entries,
                                                                       T* __restrict__ out, int64_t plane, int row0,
                                                                       int range, int64_t ntiles) {
  constexpr int N = GmChunk<T>::N;
  const int g = row0 + blockIdx.y;
  int lo = 0, hi = 0;
  if (g < range) {   // rows beyond the table (compact mode, M > range) are empty
    lo = offsets[g];
    hi = offsets[g + 1];
  }
  const float count = (float)(hi - lo);   // exact: at most 65535
  T* orow = out + (int64_t)g * plane;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t col = (tile * GM_THREADS + threadIdx.x) * N;
    if (col >= plane) return;
    const int valid = plane - col < N ? (int)(plane - col) : N;
    float acc[N];
    if (lo == hi) {
#pragma unroll
      for (int i = 0; i < N; i++) acc[i] = 0.0f;
    } else {
      gm_load<T, VEC>(src + (int64_t)entries[lo] * plane + col, valid, acc);   // starts from x[e_0], not from +0.0
      int k = lo + 1;
      for (; k + GM_UNROLL <= hi; k += GM_UNROLL) {
        float x[GM_UNROLL][N];
#pragma unroll
        for (int u = 0; u < GM_UNROLL; u++) gm_load<T, VEC>(src + (int64_t)entries[k + u] * plane + col, valid, x[u]);
#pragma unroll
        for (int u = 0; u < GM_UNROLL; u++)
#pragma unroll
          for (int i = 0; i < N; i++) acc[i] = acc[i] + x[u][i];
      }
      for (; k < hi; k++) {
        float x[N];
        gm_load<T, VEC>(src + (int64_t)entries[k] * plane + col, valid, x);
#pragma unroll
        for (int i = 0; i < N; i++) acc[i] = acc[i] + x[i];
      }
#pragma unroll
      for (int i = 0; i < N; i++) acc[i] = __fdiv_rn(acc[i], count);   // one correctly rounded division
    }
    if (VEC) {
      uint4 raw;
      T* e = reinterpret_cast<T*>(&raw);
#pragma unroll
      for (int i = 0; i < N; i++) gm_narrow(acc[i], e + i);
      *reinterpret_cast<uint4*>(orow + col) = raw;
    } else {
#pragma unroll
      for (int i = 0; i < N; i++)
        if (i < valid) gm_narrow(acc[i], orow + col + i);
    }
  }
}

template <typename T>
static void launch_reduce(const void* src, const int* offsets, const int* entries, void* out, int64_t plane, int M,
                          int range, hipStream_t s) {
  constexpr int N = GmChunk<T>::N;
  const bool vec = (uintptr_t)src % 16 == 0 && (uintptr_t)out % 16 == 0 && (plane * (int64_t)sizeof(T)) % 16 == 0;
  const int64_t ntiles = (plane + (int64_t)GM_THREADS * N - 1) / ((int64_t)GM_THREADS * N);
  const unsigned gx = (unsigned)(ntiles < (1 << 30) ? ntiles : (1 << 30));
  for (int r0 = 0; r0 < M; r0 += 65535) {   // gridDim.y ends at 65535: more rows go out in slabs
    const dim3 grid(gx, (unsigned)min(M - r0, 65535));
    if (vec)
      hipLaunchKernelGGL((graph_mean_reduce_kernel<T, true>), grid, dim3(GM_THREADS), 0, s, static_cast<const T*>(src),
                         offsets, entries, static_cast<T*>(out), plane, r0, range, ntiles);
    else
      hipLaunchKernelGGL((graph_mean_reduce_kernel<T, false>), grid, dim3(GM_THREADS), 0, s, static_cast<const T*>(src),
                         offsets, entries, static_cast<T*>(out), plane, r0, range, ntiles);
  }
}

size_t graph_mean_workspace_bytes(int E, int range) { return ((size_t)range + 1 + (size_t)E) * sizeof(int); }

void launch_graph_mean(const void* src, const int64_t* index, void* out, int E, int64_t plane, int M, int range,
                       int compact, bool half, int* groups_out, void* workspace, hipStream_t s) {
  int* offsets = static_cast<int*>(workspace);
  int* entries = offsets + range + 1;
  hipLaunchKernelGGL(graph_mean_prepare_kernel, dim3(1), dim3(GM_PREP_THREADS), 0, s, index, E, range, compact, offsets,
                     entries, groups_out);
  if (half)
    launch_reduce<__half>(src, offsets, entries, out, plane, M, range, s);
  else
    launch_reduce<float>(src, offsets, entries, out, plane, M, range, s);
}

}  // namespace droid
