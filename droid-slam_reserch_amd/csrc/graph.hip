// graph.hip -- proximity-edge selection on the device: the edge list FactorGraph.add_proximity_factors hands to
// add_factors (droid_slam/factor_graph.py:315-379), and the duplicate filter add_factors applies first (:44-55),
// from the frame-distance matrix and the edges the graph already holds.  The contract is in
// include/droid_backends_hip.h (droid_proximity_edges); this file is how it is met without a host round trip.
//
// Four stream operations, whatever t is and however many edges are accepted:
//   memset    the candidate counter
//   compact   one thread per cell of the rectangle: masked distance (steps 1-2), cells with d <= thresh -- the only
//             ones the walk can ever accept -- go to a list of 64-bit keys {ordered fp32 bits, flat index}; unique
//             keys, so their arrival order does not matter.  Also clears the known-edge hash table.
//   sort      block b sorts candidates [16384 b, 16384 (b + 1)) in LDS (bitonic); blocks past the count exit.  Usually
//             block 0 has them all.
//   select    ONE workgroup.  All 16 waves: clear the suppression bitmap of the rectangle in LDS (one bit per cell,
//             set = the cell is at inf), seed it from the suppressing edges (step 3) and the forced cells, write the
//             forced edges at their closed-form offsets (step 4), insert the known edges into the hash table; when
//             there is more than one sorted run, merge the runs (merge path, ping-pong between two buffers).
//             Then wave 0 walks the sorted list 64 candidates per step (step 5): ballot the lanes whose bit is clear,
//             accept the first, the lanes set its diamond, the live lanes look at their bits again.  The walk is
//             serial in the number of ACCEPTED pairs, not in the number of candidates.  Last, all waves drop the
//             known edges with an order-preserving compaction (step 6) and write the count.
// A masked cell never becomes a candidate again and the distance of a live cell never changes, so the order the
// reference gets from sorting the modified array is the order of the keys sorted once.
#include "graph.hpp"

namespace droid {

namespace {

constexpr int SEL_THREADS = 1024;
constexpr uint64_t KEY_PAD = ~0ull;
constexpr uint64_t HASH_EMPTY = ~0ull;

struct ProxView {
  int* hdr;          // [0] number of candidates
  uint64_t* cand;    // [cells] keys, sorted in runs of PROX_CHUNK after the sort kernel
  uint64_t* cand2;   // [cells] merge target (only when cells > PROX_CHUNK)
  int64_t* es;       // [cap, 2] unfiltered result (only when n_known > 0)
  uint64_t* hash;    // [hash_size] open-addressing set of the known edges
  int hash_size;     // power of two >= 2 n_known, or 0
};

__host__ __device__ inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// fp32 -> 32 bits that order as the floats do (negative values too; -0 is folded into +0 before)
__device__ inline uint32_t ordered_bits(float d) {
  const uint32_t b = __float_as_uint(d);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ inline uint64_t hash_mix(uint64_t k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return k;
}

__device__ inline uint64_t edge_key(int64_t i, int64_t j) { return ((uint64_t)(uint32_t)i << 32) | (uint32_t)j; }

// ---------------------------------------------------------------------------------------------------- compact
__global__ __launch_bounds__(256) void prox_compact(ProxArgs a, ProxView v, int R, int C) {
  const int cells = R * C;
  const int gid = blockIdx.x * 256 + threadIdx.x;
  for (int x = gid; x < v.hash_size; x += gridDim.x * 256) v.hash[x] = HASH_EMPTY;
  bool keep = false;
  uint64_t key = 0;
  if (gid < cells) {
    const int r = gid / C, c = gid - r * C;
    const int i = r + a.t0, j = c + a.t1;
    if ((int64_t)i - a.rad >= j) {   // step 2: i - rad < j is masked (never loaded)
      float d = a.dist[(size_t)i * a.ld + j];
      if (a.bidir) d = 0.5f * (d + a.dist[(size_t)j * a.ld + i]);
      if (d == 0.0f) d = 0.0f;       // -0 -> +0: equal distances must give equal keys
      keep = d <= 100.0f && d <= a.thresh;   // NaN: false, like inf
      key = ((uint64_t)ordered_bits(d) << 32) | (uint32_t)gid;
    }
  }
  const uint64_t m = __ballot(keep);
  if (m == 0) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((unsigned long long)m) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(v.hdr, __popcll(m));
  base = __shfl(base, leader);
  if (keep) v.cand[base + __popcll(m & ((1ull << lane) - 1))] = key;   // base + rank < cells: at most one key per cell
}

// ---------------------------------------------------------------------------------------------------- sort
__global__ __launch_bounds__(SEL_THREADS) void prox_sort_chunks(ProxView v) {
  __shared__ uint64_t keys[PROX_CHUNK];
  const int n = v.hdr[0];
  const int start = blockIdx.x * PROX_CHUNK;
  if (start >= n) return;
  const int m = min(PROX_CHUNK, n - start);
  int P = 64;
  while (P < m) P <<= 1;   // <= PROX_CHUNK
  for (int x = threadIdx.x; x < P; x += SEL_THREADS) keys[x] = x < m ? v.cand[start + x] : KEY_PAD;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int x = threadIdx.x; x < (P >> 1); x += SEL_THREADS) {
        const int lo = ((x & ~(j - 1)) << 1) | (x & (j - 1));
        const int hi = lo | j;
        const uint64_t p = keys[lo], q = keys[hi];
        if ((p > q) == ((lo & k) == 0)) { keys[lo] = q; keys[hi] = p; }
      }
      __syncthreads();
    }
  for (int x = threadIdx.x; x < m; x += SEL_THREADS) v.cand[start + x] = keys[x];
}

// ---------------------------------------------------------------------------------------------------- select
// bit of cell (r, c) of the rectangle; rows are `pitch` words
__device__ inline void bm_set(uint32_t* bm, int pitch, int r, int c) { atomicOr(&bm[r * pitch + (c >> 5)], 1u << (c & 31)); }
__device__ inline bool bm_get(const uint32_t* bm, int pitch, int r, int c) {
  return (__hip_atomic_load(&bm[r * pitch + (c >> 5)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> (c & 31)) & 1u;
}

// merge path: how many of the first k outputs of merge(a[0, la), b[0, lb)) come from a (keys are unique)
__device__ inline int merge_split(const uint64_t* a, int la, const uint64_t* b, int lb, int k) {
  int lo = max(0, k - lb), hi = min(k, la);
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < b[k - 1 - mid]) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(SEL_THREADS) void prox_select(ProxArgs a, ProxView v, int R, int C) {
  __shared__ uint32_t bm[PROX_MAX_CELLS / 32 + 1024];   // rows padded to whole words: cells / 32 + R words at most
  __shared__ int s_len, s_wave_tot[SEL_THREADS / 64], s_base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pitch = (C + 31) >> 5;
  const int t = a.t, t0 = a.t0, t1 = a.t1, nms = a.nms;
  int64_t* es = a.n_known > 0 ? v.es : a.out;

  for (int x = tid; x < R * pitch; x += SEL_THREADS) bm[x] = 0;
  __syncthreads();

  // step 3: the diamonds of the suppressing edges
  for (int e = tid; e < a.n_sup; e += SEL_THREADS) {
    const int64_t i = a.sup_ii[e], j = a.sup_jj[e];
    const int64_t sep = i > j ? i - j : j - i;
    const int rr = (int)max((int64_t)0, min(sep - 2, (int64_t)nms));
    for (int di = -rr; di <= rr; di++) {
      const int64_t i1 = i + di;
      if (i1 < t0 || i1 >= t) continue;
      const int w = rr - abs(di);
      for (int dj = -w; dj <= w; dj++) {
        const int64_t j1 = j + dj;
        if (j1 >= t1 && j1 < t) bm_set(bm, pitch, (int)(i1 - t0), (int)(j1 - t1));
      }
    }
  }
  // step 4: the forced edges of row i start at a closed-form offset; their cells inside the rectangle are masked
  const int64_t m = (int64_t)a.rad + 1;
  const int64_t f0 = prox_forced_before(t0, m);
  for (int i = t0 + tid; i < t; i += SEL_THREADS) {
    int64_t o = (a.stereo ? (i - t0) : 0) + 2 * (prox_forced_before(i, m) - f0);
    if (a.stereo) {
      es[2 * o] = i; es[2 * o + 1] = i; o++;
      bm_set(bm, pitch, i - t0, i - t1);   // t1 <= t0 <= i
    }
    for (int j = (int)max((int64_t)0, i - m); j < i; j++) {
      es[2 * o] = i; es[2 * o + 1] = j; o++;
      es[2 * o] = j; es[2 * o + 1] = i; o++;
      if (j >= t1) bm_set(bm, pitch, i - t0, j - t1);
    }
  }
  // step 6 preparation: the set of known edges (the table was cleared by prox_compact)
  for (int e = tid; e < a.n_known; e += SEL_THREADS) {
    const int64_t i = a.known_ii[e], j = a.known_jj[e];
    if (i < 0 || j < 0 || i >= t || j >= t) continue;   // cannot equal a result edge
    const uint64_t key = edge_key(i, j);
    uint32_t h = (uint32_t)hash_mix(key) & (v.hash_size - 1);
    for (;;) {
      const uint64_t prev = atomicCAS((unsigned long long*)&v.hash[h], (unsigned long long)HASH_EMPTY, (unsigned long long)key);
      if (prev == HASH_EMPTY || prev == key) break;
      h = (h + 1) & (v.hash_size - 1);   // ends: the table has >= 2 n_known slots
    }
  }

  // more candidates than one LDS sort takes: merge the sorted runs
  const int n = v.hdr[0];
  const uint64_t* sorted = v.cand;
  if (n > PROX_CHUNK) {
    uint64_t* src = v.cand;
    uint64_t* dst = v.cand2;
    const int S = (n + SEL_THREADS - 1) / SEL_THREADS;   // outputs per thread and pass, <= PROX_MAX_CELLS / 1024
    for (int64_t run = PROX_CHUNK; run < n; run <<= 1) {
      int o = tid * S;
      const int end = min(n, o + S);
      while (o < end) {
        const int ps = (int)((o / (2 * run)) * (2 * run));
        const int la = (int)min(run, (int64_t)n - ps), lb = (int)min(run, (int64_t)n - ps - la);
        const uint64_t *pa = src + ps, *pb = pa + la;
        const int k1 = min(end, ps + la + lb) - ps;
        int k = o - ps;
        int x = merge_split(pa, la, pb, lb, k), y = k - x;
        for (; k < k1; k++) {
          const bool from_a = y >= lb || (x < la && pa[x] < pb[y]);
          dst[ps + k] = from_a ? pa[x++] : pb[y++];
        }
        o = ps + k1;
      }
      __syncthreads();
      uint64_t* tmp = src; src = dst; dst = tmp;
    }
    sorted = src;
  }
  __syncthreads();

  // step 5: the walk
  const int64_t forced = prox_forced_edges(t, t0, a.rad, a.stereo);
  if (wave == 0) {
    int64_t len = forced;
    const int side = 2 * nms + 1;
    uint64_t next = lane < n ? sorted[lane] : KEY_PAD;
    bool stop = false;
    for (int pos = 0; pos < n && !stop; pos += 64) {
      const uint64_t key = next;
      next = pos + 64 + lane < n ? sorted[pos + 64 + lane] : KEY_PAD;   // the next step's keys are on their way
      const int flat = key != KEY_PAD ? (int)(uint32_t)key : 0;
      const int r = flat / C, c = flat - r * C;
      bool live = key != KEY_PAD && !bm_get(bm, pitch, r, c);
      for (;;) {
        const uint64_t mask = __ballot(live);
        if (mask == 0) break;
        if (len > a.max_factors) { stop = true; break; }
        const int first = __ffsll((unsigned long long)mask) - 1;
        const int i = __shfl(r, first) + t0, j = __shfl(c, first) + t1;
        if (lane == 0) { es[2 * len] = i; es[2 * len + 1] = j; es[2 * len + 2] = j; es[2 * len + 3] = i; }
        len += 2;
        const int rr = max(min(abs(i - j) - 2, nms), 0);   // rr = 0: the cell itself
        for (int q = lane; q < side * side; q += 64) {
          const int di = q / side - nms, dj = q - (q / side) * side - nms;
          const int i1 = i + di, j1 = j + dj;
          if (abs(di) + abs(dj) <= rr && i1 >= t0 && i1 < t && j1 >= t1 && j1 < t) bm_set(bm, pitch, i1 - t0, j1 - t1);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // one wave: LDS operations retire in order
        live = live && !bm_get(bm, pitch, r, c);
      }
    }
    if (lane == 0) s_len = (int)len;
  }
  __syncthreads();
  const int len = s_len;
  if (a.n_known <= 0) {
    if (tid == 0) *a.count_out = len;
    return;
  }

  // step 6: drop the known edges, keep the order
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int e0 = 0; e0 < len; e0 += SEL_THREADS) {
    const int e = e0 + tid;
    bool keep = false;
    int64_t i = 0, j = 0;
    if (e < len) {
      i = es[2 * e]; j = es[2 * e + 1];
      const uint64_t key = edge_key(i, j);
      uint32_t h = (uint32_t)hash_mix(key) & (v.hash_size - 1);
      keep = true;
      for (;;) {
        const uint64_t got = __hip_atomic_load(&v.hash[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (got == HASH_EMPTY) break;
        if (got == key) { keep = false; break; }
        h = (h + 1) & (v.hash_size - 1);
      }
    }
    const uint64_t mask = __ballot(keep);
    if (lane == 0) s_wave_tot[wave] = __popcll(mask);
    __syncthreads();
    int before = s_base;
    for (int w = 0; w < wave; w++) before += s_wave_tot[w];
    if (keep) {
      const int o = before + __popcll(mask & ((1ull << lane) - 1));
      a.out[2 * o] = i; a.out[2 * o + 1] = j;
    }
    __syncthreads();
    if (tid == SEL_THREADS - 1) s_base = before + __popcll(mask);   // the last wave's end = the chunk's end
    __syncthreads();
  }
  if (tid == 0) *a.count_out = s_base;
}

size_t carve(ProxView& v, void* ws, int t, int t0, int t1, int n_known, int cap) {
  const size_t cells = t > t0 ? (size_t)(t - t0) * (size_t)(t - t1) : 0;
  char* p = (char*)ws;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* q = p ? p + off : nullptr; off += up256(bytes); return q; };
  v.hdr = (int*)take(16);
  v.cand = (uint64_t*)take(cells * 8);
  v.cand2 = (uint64_t*)take(cells > (size_t)PROX_CHUNK ? cells * 8 : 0);
  v.hash_size = 0;
  if (n_known > 0) {
    v.hash_size = 64;
    while ((int64_t)v.hash_size < 2 * (int64_t)n_known) v.hash_size <<= 1;
  }
  v.es = (int64_t*)take(n_known > 0 ? (size_t)cap * 16 : 0);
  v.hash = (uint64_t*)take((size_t)v.hash_size * 8);
  return off;
}

}  // namespace

size_t prox_workspace_bytes(int t, int t0, int t1, int n_known, int cap) {
  ProxView v;
  return carve(v, nullptr, t, t0, t1, n_known, cap);
}

void launch_proximity_edges(const ProxArgs& a, hipStream_t s) {
  if (a.t <= a.t0) {   // no rows: no forced edges, no candidates
    (void)hipMemsetAsync(a.count_out, 0, sizeof(int), s);
    return;
  }
  ProxView v;
  carve(v, a.ws, a.t, a.t0, a.t1, a.n_known, a.cap);
  const int R = a.t - a.t0, C = a.t - a.t1, cells = R * C;
  (void)hipMemsetAsync(v.hdr, 0, 16, s);
  hipLaunchKernelGGL(prox_compact, dim3((cells + 255) / 256), dim3(256), 0, s, a, v, R, C);
  hipLaunchKernelGGL(prox_sort_chunks, dim3((cells + PROX_CHUNK - 1) / PROX_CHUNK), dim3(SEL_THREADS), 0, s, v);
  hipLaunchKernelGGL(prox_select, dim3(1), dim3(SEL_THREADS), 0, s, a, v, R, C);
}

}  // namespace droid
