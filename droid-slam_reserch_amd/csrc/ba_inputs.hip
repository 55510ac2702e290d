// ba_inputs.hip -- the tail of `FactorGraph.update` between the update operator and `ba` (droid_slam/factor_graph.py:
// 213-238; the per-step tail of update_lowmem, :292-294) as two launches on one stream: a one-workgroup prepare that
// turns the index lists into the emitted edge list, the frame lists and per-row source tables, and a streaming launch
// that reads every input row once and writes every output row once.  The contract (edge list, arithmetic, limits) is in
// include/droid_update_hip.h (droid_ba_inputs); resource figures and timings: DESIGN.md.  No atomics anywhere.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/droid_update_hip.h"
#include "launchers.hpp"

// eta = fl(fl(0.2f * d) + ep) is two roundings by contract.  hipcc's default -ffp-contract=fast fuses the pair into one
// fma, also when it is written with __fmul_rn / __fadd_rn: they are inline functions of a header compiled with
// contraction on, and their operators fuse once inlined.  So contraction is off for this file and the pair is written
// with plain operators.
#pragma clang fp contract(off)

namespace droid {

// --------------------------------------------------------------------------------------------------- workspace layout
// ints: head[BI_HEAD] = {Eb, M, ...}; src_row [E + Ei]: the input row of BA row r, e >= 0 for active edge e and -1 - k
// for inactive edge k; eta_frame [mcap]: the frame of eta row i; eta_src [mcap]: its row of damping_net, or -1 for the
// stored damping_buf row.  mcap = min(nbuf, E + Ei).
constexpr int BI_HEAD = 4;
static inline int bi_mcap(int E, int Ei, int nbuf) { return nbuf < E + Ei ? nbuf : E + Ei; }

size_t ba_inputs_workspace_bytes(int E, int Ei, int nbuf) {
  return ((size_t)BI_HEAD + (size_t)(E + Ei) + 2 * (size_t)bi_mcap(E, Ei, nbuf)) * sizeof(int);
}

// ------------------------------------------------------------------------------------------------------------- prepare
// One workgroup of 1024 threads.  LDS: a presence byte per frame for the active and for the kept inactive sources (a
// plain byte store of 1: threads that meet at a frame store the same value), the two bitmaps packed from them with their
// prefix ranks (one word per thread: nbuf <= 16384), and 1024 int64 slots for the min / max reductions.
constexpr int BI_PREP_THREADS = 1024;
constexpr int BI_WORDS = DROID_BA_INPUTS_MAX_NBUF / 32;

__device__ __forceinline__ int bi_block_exclusive_scan(int x, int* wave_sums /*[16] LDS*/, int* total) {
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
  for (int w = 0; w < BI_PREP_THREADS / 64; w++) {
    const int s = wave_sums[w];
    if (w < wave) base += s;
    sum += s;
  }
  *total = sum;
  return base + inc - x;
}

// min (MAX = false) or max over one int64 per thread; every thread calls it and gets the result
template <bool MAX>
__device__ __forceinline__ int64_t bi_block_extreme(int64_t x, int64_t* slots /*[1024] LDS*/) {
  __syncthreads();   // slots may still be read from an earlier reduction
  slots[threadIdx.x] = x;
  __syncthreads();
  for (int n = BI_PREP_THREADS / 2; n > 0; n >>= 1) {
    if ((int)threadIdx.x < n) {
      const int64_t a = slots[threadIdx.x], b = slots[threadIdx.x + n];
      slots[threadIdx.x] = MAX ? (a > b ? a : b) : (a < b ? a : b);
    }
    __syncthreads();
  }
  return slots[0];
}

__device__ __forceinline__ int bi_saturate(int64_t v) { return v > INT_MAX ? INT_MAX : v < INT_MIN ? INT_MIN : (int)v; }

struct BiPrep {
  const int64_t *ii, *jj, *ii_inac, *jj_inac;
  int E, Ei, nbuf, n_damp, has_damping, t0;
  int64_t *ii_ba, *jj_ba, *frames_active, *frames_eta;
  int *info, *head, *src_row, *eta_frame, *eta_src;
};

__global__ __launch_bounds__(BI_PREP_THREADS) void ba_inputs_prepare_kernel(BiPrep p) {
  __shared__ uint8_t in_a[DROID_BA_INPUTS_MAX_NBUF], in_i[DROID_BA_INPUTS_MAX_NBUF];
  __shared__ uint32_t bits_a[BI_WORDS], bits_u[BI_WORDS];
  __shared__ int rank_a[BI_WORDS], rank_u[BI_WORDS];
  __shared__ int64_t slots[BI_PREP_THREADS];
  __shared__ int wave_sums[BI_PREP_THREADS / 64];
  const int t = threadIdx.x;
  const int E = p.E, Ei = p.Ei, nbuf = p.nbuf;
  const int nwords = (nbuf + 31) >> 5;

  for (int v = t; v < nwords * 32; v += BI_PREP_THREADS) in_a[v] = in_i[v] = 0;   // nwords * 32 <= 16384

  // 1. t0'
  int64_t t0 = p.t0;
  if (p.t0 < 0) {
    int64_t lo = INT64_MAX;
    for (int e = t; e < E; e += BI_PREP_THREADS) {
      const int64_t v = p.ii[e];
      lo = v < lo ? v : lo;
    }
    lo = bi_block_extreme<false>(lo, slots);
    t0 = lo >= 1 ? (lo == INT64_MAX ? lo : lo + 1) : 1;
  }
  const int64_t thr = t0 - 3;

  // 2. the kept inactive edges in their order: thread t owns inactive edges [k0, k1)
  const int per = (Ei + BI_PREP_THREADS - 1) / BI_PREP_THREADS;
  const int k0 = min(t * per, Ei), k1 = min(k0 + per, Ei);
  int mine = 0;
  for (int k = k0; k < k1; k++) mine += (p.ii_inac[k] >= thr && p.jj_inac[k] >= thr) ? 1 : 0;
  int K;
  int pos = bi_block_exclusive_scan(mine, wave_sums, &K);   // its barriers also publish the cleared presence bytes
  int64_t hi = INT64_MIN;
  int outside = 0;
  for (int k = k0; k < k1; k++) {
    const int64_t a = p.ii_inac[k], b = p.jj_inac[k];
    if (a >= thr && b >= thr) {
      p.ii_ba[pos] = a;
      p.jj_ba[pos] = b;
      p.src_row[pos] = -1 - k;
      pos++;
      hi = a > hi ? a : hi;
      hi = b > hi ? b : hi;
      if (a >= 0 && a < nbuf) in_i[a] = 1;
      outside |= (a < 0 || a >= nbuf || b < 0 || b >= nbuf) ? 1 : 0;
    }
  }
  // 3. then the active edges
  for (int e = t; e < E; e += BI_PREP_THREADS) {
    const int64_t a = p.ii[e], b = p.jj[e];
    p.ii_ba[K + e] = a;
    p.jj_ba[K + e] = b;
    p.src_row[K + e] = e;
    hi = a > hi ? a : hi;
    hi = b > hi ? b : hi;
    if (a >= 0 && a < nbuf) in_a[a] = 1;
    outside |= (a < 0 || a >= nbuf || b < 0 || b >= nbuf) ? 1 : 0;
  }
  hi = bi_block_extreme<true>(hi, slots);   // its barriers also publish the presence bytes
  outside = __syncthreads_or(outside);

  // 4. bitmaps, their ranks, the two frame lists and the source of every eta row
  int pa = 0, pu = 0;
  if (t < nwords) {
    uint32_t wa = 0, wi = 0;
    for (int b = 0; b < 32; b++) {
      wa |= (uint32_t)in_a[t * 32 + b] << b;
      wi |= (uint32_t)in_i[t * 32 + b] << b;
    }
    bits_a[t] = wa;
    bits_u[t] = wa | wi;
    pa = __popc(wa);
    pu = __popc(wa | wi);
  }
  int G, M;
  const int ra = bi_block_exclusive_scan(pa, wave_sums, &G);
  const int ru = bi_block_exclusive_scan(pu, wave_sums, &M);
  if (t < nwords) {
    rank_a[t] = ra;
    rank_u[t] = ru;
  }
  __syncthreads();
  for (int v = t; v < nbuf; v += BI_PREP_THREADS) {
    const uint32_t wa = bits_a[v >> 5], wu = bits_u[v >> 5], below = (1u << (v & 31)) - 1u;
    if (!((wu >> (v & 31)) & 1u)) continue;
    const int i = rank_u[v >> 5] + __popc(wu & below);
    int src = -1;
    if ((wa >> (v & 31)) & 1u) {
      const int g = rank_a[v >> 5] + __popc(wa & below);
      p.frames_active[g] = v;
      if (p.has_damping && g < p.n_damp) src = g;
    }
    p.frames_eta[i] = v;
    p.eta_frame[i] = v;
    p.eta_src[i] = src;
  }

  // 5. the record the host may read, and the counts the streaming launch reads
  if (t == 0) {
    const int flags = (outside ? 1 : 0) | ((p.has_damping && p.n_damp != G) ? 2 : 0);
    p.info[0] = K + E;
    p.info[1] = M;
    p.info[2] = G;
    p.info[3] = bi_saturate(t0);
    p.info[4] = bi_saturate(hi == INT64_MAX ? hi : hi + 1);
    p.info[5] = flags;
    p.info[6] = K;
    p.info[7] = 0;
    p.head[0] = K + E;
    p.head[1] = M;
    p.head[2] = G;
    p.head[3] = K;
  }
}

// -------------------------------------------------------------------------------------------------------------- stream
// grid (rows, tiles of the plane): rows [0, E + Ei) are BA rows, the rest eta rows; a row beyond the device count exits
// at once.  A thread owns BI_PX pixels of the row.  Where every pointer of the row is 16-byte aligned (8 for four
// halves) and the four pixels lie inside the plane it moves them with 16-byte loads of the interleaved inputs and one
// 16-byte store per plane; otherwise the same thread handles the same pixels one by one.  The arithmetic per element is
// the same, so are the bits.  No LDS.
constexpr int BI_THREADS = 256;
constexpr int BI_PX = 4;

__device__ __forceinline__ float bi_widen(__half x) { return __half2float(x); }   // exact, subnormals kept
__device__ __forceinline__ float bi_widen(float x) { return x; }

__device__ __forceinline__ bool bi_aligned(const void* p, int bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }

// n consecutive elements of T widened to float; `vec`: p is aligned to n * sizeof(T) (8, 16 or 32 bytes)
template <typename T, int N>
__device__ __forceinline__ void bi_load(const T* __restrict__ p, bool vec, int valid, float (&x)[N]) {
  if (vec) {
    constexpr int CH = 16 / sizeof(T) < N ? 16 / sizeof(T) : N;   // elements per load
    using Raw = typename std::conditional<CH * sizeof(T) == 16, uint4, uint2>::type;
#pragma unroll
    for (int c = 0; c < N / CH; c++) {
      const Raw raw = *reinterpret_cast<const Raw*>(p + c * CH);
      const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
      for (int i = 0; i < CH; i++) x[c * CH + i] = bi_widen(e[i]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; i++) x[i] = i < valid ? bi_widen(p[i]) : 0.0f;
  }
}

template <int N>
__device__ __forceinline__ void bi_store(float* __restrict__ p, bool vec, int valid, const float (&x)[N]) {
  if (vec) {
#pragma unroll
    for (int c = 0; c < N / 4; c++)
      *reinterpret_cast<float4*>(p + 4 * c) = make_float4(x[4 * c], x[4 * c + 1], x[4 * c + 2], x[4 * c + 3]);
  } else {
#pragma unroll
    for (int i = 0; i < N; i++)
      if (i < valid) p[i] = x[i];
  }
}

struct BiStream {
  const float* a;
  const void *delta, *w, *damping_net;
  float* damping_buf;
  const float *target_inac, *weight_inac;
  float *target_state, *weight_state, *target_ba, *weight_ba, *eta;
  const int *head, *src_row, *eta_frame, *eta_src;
  int rows_e;   // E + Ei: the rows before the eta rows
  int64_t hw;
  float ep;
};

// TN: dtype of delta and (in absorb mode) w; TD: dtype of damping_net
template <typename TN, typename TD>
__global__ __launch_bounds__(BI_THREADS) void ba_inputs_stream_kernel(BiStream p, int64_t ntiles) {
  const int row = blockIdx.x;
  const int64_t hw = p.hw;
  if (row < p.rows_e) {
    if (row >= p.head[0]) return;
    const int src = p.src_row[row];
    const bool active = src >= 0, absorb = p.delta != nullptr;
    const int64_t in_off = (int64_t)(active ? src : -1 - src) * hw * 2;
    const float* a = (active ? p.a : p.target_inac) + in_off;
    const bool net = active && absorb;   // the row adds the network's delta and widens its weight
    const float* wf = net ? nullptr : (active ? static_cast<const float*>(p.w) : p.weight_inac) + in_off;   // fp32 weights
    const TN* wn = net ? static_cast<const TN*>(p.w) + in_off : nullptr;
    const TN* dl = net ? static_cast<const TN*>(p.delta) + in_off : nullptr;
    float* ts = net && p.target_state ? p.target_state + in_off : nullptr;
    float* wsr = net && p.weight_state ? p.weight_state + in_off : nullptr;
    float* tb = p.target_ba + (int64_t)row * hw * 2;
    float* wb = p.weight_ba + (int64_t)row * hw * 2;
    bool vec = bi_aligned(a, 16) && bi_aligned(tb, 16) && bi_aligned(wb, 16) && hw % 4 == 0;   // both planes aligned
    vec = vec && (net ? bi_aligned(wn, 16) && bi_aligned(dl, 16) : bi_aligned(wf, 16));
    vec = vec && (!ts || bi_aligned(ts, 16)) && (!wsr || bi_aligned(wsr, 16));
    for (int64_t tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
      const int64_t px = (tile * BI_THREADS + threadIdx.x) * BI_PX;
      if (px >= hw) return;
      const int valid = hw - px < BI_PX ? (int)(hw - px) : BI_PX;   // pixels
      const bool v = vec && valid == BI_PX;
      float t[2 * BI_PX], wt[2 * BI_PX];
      bi_load<float, 2 * BI_PX>(a + 2 * px, v, 2 * valid, t);
      if (net) {
        float d[2 * BI_PX];
        bi_load<TN, 2 * BI_PX>(dl + 2 * px, v, 2 * valid, d);
        bi_load<TN, 2 * BI_PX>(wn + 2 * px, v, 2 * valid, wt);
#pragma unroll
        for (int i = 0; i < 2 * BI_PX; i++) t[i] = t[i] + d[i];
        if (ts) bi_store<2 * BI_PX>(ts + 2 * px, v, 2 * valid, t);
        if (wsr) bi_store<2 * BI_PX>(wsr + 2 * px, v, 2 * valid, wt);
      } else {
        bi_load<float, 2 * BI_PX>(wf + 2 * px, v, 2 * valid, wt);
      }
#pragma unroll
      for (int c = 0; c < 2; c++) {
        float tp[BI_PX], wp[BI_PX];
#pragma unroll
        for (int i = 0; i < BI_PX; i++) {
          tp[i] = t[2 * i + c];
          wp[i] = wt[2 * i + c];
        }
        bi_store<BI_PX>(tb + c * hw + px, v, valid, tp);
        bi_store<BI_PX>(wb + c * hw + px, v, valid, wp);
      }
    }
    return;
  }
  const int i = row - p.rows_e;
  if (i >= p.head[1]) return;
  const int64_t f = p.eta_frame[i];
  const int g = p.eta_src[i];
  float* buf = p.damping_buf + f * hw;
  const TD* dn = g < 0 ? nullptr : static_cast<const TD*>(p.damping_net) + (int64_t)g * hw;
  float* out = p.eta + (int64_t)i * hw;
  const bool vec = bi_aligned(buf, 16) && bi_aligned(out, 16) && (g < 0 || bi_aligned(dn, BI_PX * (int)sizeof(TD)));
  for (int64_t tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
    const int64_t px = (tile * BI_THREADS + threadIdx.x) * BI_PX;
    if (px >= hw) return;
    const int valid = hw - px < BI_PX ? (int)(hw - px) : BI_PX;
    const bool v = vec && valid == BI_PX;
    float d[BI_PX];
    if (g >= 0) {
      bi_load<TD, BI_PX>(dn + px, v, valid, d);
      bi_store<BI_PX>(buf + px, v, valid, d);
    } else {
      bi_load<float, BI_PX>(buf + px, v, valid, d);
    }
#pragma unroll
    for (int k = 0; k < BI_PX; k++) {   // two roundings, never an fma (contraction is off above)
      const float prod = 0.2f * d[k];
      d[k] = prod + p.ep;
    }
    bi_store<BI_PX>(out + px, v, valid, d);
  }
}

void launch_ba_inputs(const BaInputsArgs& x, hipStream_t s) {
  int* head = static_cast<int*>(x.workspace);
  int* src_row = head + BI_HEAD;
  int* eta_frame = src_row + (x.E + x.Ei);
  const int mcap = bi_mcap(x.E, x.Ei, x.nbuf);
  int* eta_src = eta_frame + mcap;
  BiPrep p{x.ii, x.jj, x.ii_inac, x.jj_inac, x.E, x.Ei, x.nbuf, x.n_damp, x.damping_net != nullptr, x.t0,
           x.ii_ba, x.jj_ba, x.frames_active, x.frames_eta, x.info, head, src_row, eta_frame, eta_src};
  hipLaunchKernelGGL(ba_inputs_prepare_kernel, dim3(1), dim3(BI_PREP_THREADS), 0, s, p);

  BiStream q{x.a, x.delta, x.w, x.damping_net, x.damping_buf, x.target_inac, x.weight_inac, x.target_state,
             x.weight_state, x.target_ba, x.weight_ba, x.eta, head, src_row, eta_frame, eta_src, x.E + x.Ei,
             (int64_t)x.H * x.W, x.ep};
  const int64_t ntiles = (q.hw + (int64_t)BI_THREADS * BI_PX - 1) / ((int64_t)BI_THREADS * BI_PX);
  // rows on grid.x (at most 65535 + 16384 of its 2^31 - 1), tiles on grid.y, which ends at 65535: a block walks the rest
  const dim3 grid((unsigned)(x.E + x.Ei + mcap), (unsigned)(ntiles < 65535 ? ntiles : 65535));
  const bool hn = x.net_half, hd = x.damp_half;
  if (hn && hd)
    hipLaunchKernelGGL((ba_inputs_stream_kernel<__half, __half>), grid, dim3(BI_THREADS), 0, s, q, ntiles);
  else if (hn)
    hipLaunchKernelGGL((ba_inputs_stream_kernel<__half, float>), grid, dim3(BI_THREADS), 0, s, q, ntiles);
  else if (hd)
    hipLaunchKernelGGL((ba_inputs_stream_kernel<float, __half>), grid, dim3(BI_THREADS), 0, s, q, ntiles);
  else
    hipLaunchKernelGGL((ba_inputs_stream_kernel<float, float>), grid, dim3(BI_THREADS), 0, s, q, ntiles);
}

}  // namespace droid
