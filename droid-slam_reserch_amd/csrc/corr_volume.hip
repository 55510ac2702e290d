// corr_volume.hip -- corr_volume_pyramid: CorrBlock.__init__ (droid_slam/modules/corr.py:24-38, 63-71) for a list of
// edges in ONE launch, from the feature buffer as DepthVideo holds it (depth_video.py:44, channels first).  Not one of
// the reference's nine operators; the contract is in include/droid_backends_hip.h (droid_corr_volume_pyramid).
//
//   a = T(fmaps[ii[e], 0] / 4), b = T(fmaps[jj[e], cam] / 4)              (T = the dtype of fmaps, rounded first)
//   level 0    vol0[e, p, q] = T(sum_c a[c, p] * b[c, q])                 (fp32 products and sum)
//   level l+1  = T(fp32(((v00 + v01) + v10) + v11) * 0.25f) of the ROUNDED level l over the (h2, w2) plane
//
// The stock sequence writes level 0, reads it back for level 1, and so on (2.64x the bytes of level 0) and gathers
// and scales the feature maps first; here a workgroup owns P query pixels p and walks the (h2, w2) plane in tiles of
// 8 rows x up to 64 columns, so that every 8x8 block a level-3 cell pools lies inside one tile.  Per tile:
//   1. the K x tile slab of b is staged in chunks of KC channels, coalesced along the plane ([k][q] rows, as it lies
//      in memory) and scaled on the way;
//   2. the plane index q is the MFMA ROW: half = v_mfma_f32_16x16x32_f16 whose [q][k] operand comes out of the
//      K-major image through ds_read_b64_tr_b16; fp32 = v_mfma_f32_16x16x4_f32 (exact fp32 products, plain reads);
//   3. the accumulators are rounded to T into a [p][q] image that reuses the staging buffer; level 0 leaves from
//      there in 16-byte pieces (a whole 8 x w run per p when w <= 64), and one thread per (p, 8x8 block) pools
//      levels 1-3 in registers from the rounded values.  Level 0 never comes back from memory.
// a (P pixels x C) is transposed into LDS once per workgroup.  No atomics; an edge's bits do not depend on E or slot.
// The slot of edge e is slot0 + e, or slots[e] when a slot list is given (droid_corr_volume_pyramid_slots).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/droid_backends_hip.h"
#include "launchers.hpp"

namespace droid {

typedef _Float16 cv_h8 __attribute__((ext_vector_type(8)));
typedef short cv_s4 __attribute__((ext_vector_type(4)));
typedef float cv_f4 __attribute__((ext_vector_type(4)));

struct CvArgs {
  const void* fmaps;
  const int64_t* ii;
  const int64_t* jj;
  void* out[4];
  int E, nbuf, ncam, C, H, W, levels;
  long long slot0;        // edge e -> slot slot0 + e, or
  const int64_t* slots;   // (not null) -> slot slots[e]; outside [0, cap) the edge is skipped
  long long cap;
  int nptiles, nbands, nxc;
};

constexpr int CV_QS = 528;   // row pitch of the [k][q] image: 512 + 16 elements (rows 8 banks apart, see cv_krow)
constexpr int CV_OS = 520;   // row pitch of the [p][q] image
constexpr int CV_AS = 264;   // row pitch of the [p][k] image of a (C <= 256)
constexpr int CV_MT = 8;     // 16-row MFMA tiles per wave and plane tile: 4 waves x 8 x 16 = 512 = 8 rows x 64 columns

template <typename T> struct CvCfg;
template <> struct CvCfg<_Float16> { static constexpr int P = 32, KC = 32; };
template <> struct CvCfg<float> { static constexpr int P = 16, KC = 16; };

// Row of channel k (0..31) of a chunk in the half [k][q] image.  One transposed read of a 32-lane half takes the
// channel blocks {8g .. 8g+3} (or +4) of g = 0, 1; with rows 8 banks apart the blocks k and k + 8 would share
// banks, so bits 2 and 3 of k change places: every half-wave read then covers eight rows that differ mod 8.
__device__ __forceinline__ int cv_krow(int k) { return (k & 19) | ((k & 4) << 1) | ((k & 8) >> 1); }

__device__ __forceinline__ unsigned cv_virtual_id() {   // XCD-aware order: the p-tiles of one edge share an L2
  const unsigned total = gridDim.x;
  unsigned v = blockIdx.x;
  if ((total & 7u) == 0) v = (v & 7u) * (total >> 3) + (v >> 3);
  return v;
}

template <typename T>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 2 : 1) void corr_volume_pyramid_kernel(const CvArgs a) {
  constexpr int P = CvCfg<T>::P, KC = CvCfg<T>::KC, NT = P / 16;
  constexpr int V = 16 / (int)sizeof(T);   // elements of a 16-byte piece
  constexpr bool HALF = sizeof(T) == 2;
  constexpr int BQ = (KC * CV_QS > P * CV_OS ? KC * CV_QS : P * CV_OS);
  __shared__ __attribute__((aligned(16))) T lds_bq[BQ];          // [k][q] chunk of b, then the [p][q] result
  __shared__ __attribute__((aligned(16))) T lds_a[P * CV_AS];    // [p][k] image of a

  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned v = cv_virtual_id();
  const int e = (int)(v / (unsigned)a.nptiles), pt = (int)(v % (unsigned)a.nptiles);
  const int H = a.H, W = a.W, C = a.C;
  const size_t hw = (size_t)H * W;
  const long long fi = a.ii[e], fj = a.jj[e];
  const bool valid = fi >= 0 && fi < a.nbuf && fj >= 0 && fj < a.nbuf;   // else zeros, like altcorr_pyramid_forward
  const int cam = (a.ncam == 2 && fi == fj) ? 1 : 0;
  const T* fa = (const T*)a.fmaps + (valid ? (size_t)fi * a.ncam * C * hw : 0);
  const T* fb = (const T*)a.fmaps + (valid ? ((size_t)fj * a.ncam + cam) * C * hw : 0);
  const int p0 = pt * P;
  long long eslot = a.slot0 + e;
  if (a.slots) {   // uniform over the workgroup (one scalar load): a skipped edge leaves before any barrier
    eslot = a.slots[e];
    if (eslot < 0 || eslot >= a.cap) return;
  }
  const size_t slot = (size_t)eslot;
  const T quarter = (T)0.25f;

  // a: [c][p] in memory -> [p][c], scaled.  T(x * 0.25) is the correctly rounded x / 4 (subnormal results included).
  for (int idx = tid; idx < P * C; idx += 256) {
    const int k = idx / P, p = idx % P;
    T x = (T)0;
    if (valid && (size_t)(p0 + p) < hw) x = fa[(size_t)k * hw + p0 + p] * quarter;
    lds_a[p * CV_AS + k] = x;
  }

  // Staging map of the 256 threads over a KC x [8][wc] chunk, free of divisions: 64 / V consecutive lanes cover one
  // plane row in 16-byte pieces (lanes past the tile's width idle), 8 rows, KPI channels per pass, 8 passes.  The same
  // map with query pixels in place of channels serves the level-0 store.
  constexpr int PXB = 64 / V, KPI = 256 / (8 * PXB), NPASS = KC / KPI;
  static_assert(NPASS == 8 && P / KPI == 8, "eight passes for the staging and for the level-0 store");
  const int s_px = (tid % PXB) * V, s_r = (tid / PXB) & 7, s_k = tid / (8 * PXB);
  const int ntiles = a.nbands * a.nxc;
  uint4 raw[NPASS];   // the chunk in flight: requested one chunk ahead, behind the products of the current one
  auto request = [&](int t, int kc) {
    const int band = t / a.nxc, x0 = (t % a.nxc) * 64;
    const int wc = min(64, W - x0), y = 8 * band + s_r;
    const bool live = valid && y < H && s_px < wc;
    const T* src = fb + (size_t)(kc + s_k) * hw + (size_t)y * W + x0 + s_px;
#pragma unroll
    for (int it = 0; it < NPASS; it++) {
      raw[it] = make_uint4(0, 0, 0, 0);
      if (live) raw[it] = *(const uint4*)(src + (size_t)(it * KPI) * hw);
    }
  };
  request(0, 0);

  for (int t = 0; t < ntiles; t++) {
    const int band = t / a.nxc, x0 = (t % a.nxc) * 64;
    const int wc = min(64, W - x0);      // columns of this tile (a multiple of 8)
    const int QP = 8 * wc;               // plane positions of this tile, row-major [8][wc]
    const int nmt = QP >> 4;             // 16-row MFMA tiles (QP is a multiple of 64)
    cv_f4 acc[CV_MT][NT];
#pragma unroll
    for (int i = 0; i < CV_MT; i++)
#pragma unroll
      for (int n = 0; n < NT; n++) acc[i][n] = cv_f4{0.f, 0.f, 0.f, 0.f};

    for (int kc = 0; kc < C; kc += KC) {
      __syncthreads();   // the image is free: the last chunk's products / the last tile's stores are done
      if (s_px < wc) {
#pragma unroll
        for (int it = 0; it < NPASS; it++) {
          const int kk = s_k + it * KPI;
          if constexpr (HALF) {
            cv_h8 h = __builtin_bit_cast(cv_h8, raw[it]);
            h = h * (_Float16)0.25f;
            *(cv_h8*)(lds_bq + cv_krow(kk) * CV_QS + s_r * wc + s_px) = h;
          } else {
            cv_f4 f = __builtin_bit_cast(cv_f4, raw[it]);
            f = f * 0.25f;
            *(cv_f4*)(lds_bq + kk * CV_QS + s_r * wc + s_px) = f;
          }
        }
      }
      __syncthreads();
      if (kc + KC < C) request(t, kc + KC);
      else if (t + 1 < ntiles) request(t + 1, 0);
      if constexpr (HALF) {
        const int g = lane >> 4, i16 = lane & 15;
        cv_h8 bf[NT];
#pragma unroll
        for (int n = 0; n < NT; n++) bf[n] = *(const cv_h8*)(lds_a + (n * 16 + i16) * CV_AS + kc + 8 * g);
        // lane 4q + p of a 16-lane group addresses row q, columns 4p .. 4p+3 of a 4-channel x 16-position block and
        // receives position (lane & 15) of the four channels: channels 8g .. 8g+3, then 8g+4 .. 8g+7
        const int klo = 8 * g + (i16 >> 2);
        const T* row_lo = lds_bq + cv_krow(klo) * CV_QS + 4 * (i16 & 3);
        const T* row_hi = lds_bq + cv_krow(klo + 4) * CV_QS + 4 * (i16 & 3);
#pragma unroll
        for (int i = 0; i < CV_MT; i++) {
          const int mt = wv + 4 * i;
          if (mt < nmt) {   // wave-uniform: EXEC stays all ones for the transposed reads
            typedef __attribute__((address_space(3))) cv_s4 lds_s4;
            const cv_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(row_lo + mt * 16));
            const cv_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(row_hi + mt * 16));
            const cv_h8 af = __builtin_bit_cast(cv_h8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
            for (int n = 0; n < NT; n++) acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf[n], acc[i][n], 0, 0, 0);
          }
        }
      } else {
        const int g = lane >> 4, i16 = lane & 15;
#pragma unroll
        for (int ks = 0; ks < KC; ks += 4) {
          float bf[NT];
#pragma unroll
          for (int n = 0; n < NT; n++) bf[n] = lds_a[(n * 16 + i16) * CV_AS + kc + ks + g];
#pragma unroll
          for (int i = 0; i < CV_MT; i++) {
            const int mt = wv + 4 * i;
            if (mt < nmt) {
              const float af = lds_bq[(ks + g) * CV_QS + mt * 16 + i16];
#pragma unroll
              for (int n = 0; n < NT; n++) acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf[n], acc[i][n], 0, 0, 0);
            }
          }
        }
      }
    }

    // accumulators (row = 4 * (lane >> 4) + reg is the plane position, column = lane & 15 the query pixel) -> [p][q]
    __syncthreads();
#pragma unroll
    for (int i = 0; i < CV_MT; i++) {
      const int mt = wv + 4 * i;
      if (mt < nmt) {
#pragma unroll
        for (int n = 0; n < NT; n++) {
          T* dst = lds_bq + (n * 16 + (lane & 15)) * CV_OS + mt * 16 + 4 * (lane >> 4);
#pragma unroll
          for (int r = 0; r < 4; r++) dst[r] = (T)acc[i][n][r];
        }
      }
    }
    __syncthreads();

    // level 0: 16-byte pieces; one p's tile is one run of 8 * w elements when the tile spans the plane's width
    {
      const int y = 8 * band + s_r;
      if (s_px < wc && y < H) {
        T* dst = (T*)a.out[0] + (slot * hw + p0 + s_k) * hw + (size_t)y * W + x0 + s_px;
        const T* src = lds_bq + s_k * CV_OS + s_r * wc + s_px;
#pragma unroll
        for (int it = 0; it < 8; it++)
          if ((size_t)(p0 + s_k + it * KPI) < hw)
            *(uint4*)(dst + (size_t)(it * KPI) * hw) = *(const uint4*)(src + it * KPI * CV_OS);
      }
    }
    // levels 1-3: one thread per (p, 8x8 block), from the rounded values; an output exists iff its index < size >> l
    if (a.levels > 1) {
      const int p = tid >> 3, bx = tid & 7;
      if (p < P && 8 * bx < wc && (size_t)(p0 + p) < hw) {
        const T* src = lds_bq + p * CV_OS + 8 * bx;
        __attribute__((aligned(16))) T l1[4][4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          __attribute__((aligned(16))) T top[8];
          __attribute__((aligned(16))) T bot[8];
#pragma unroll
          for (int c = 0; c < 8; c += V) {
            *(uint4*)(top + c) = *(const uint4*)(src + (2 * r) * wc + c);
            *(uint4*)(bot + c) = *(const uint4*)(src + (2 * r + 1) * wc + c);
          }
#pragma unroll
          for (int c = 0; c < 4; c++)
            l1[r][c] = (T)(((((float)top[2 * c] + (float)top[2 * c + 1]) + (float)bot[2 * c]) + (float)bot[2 * c + 1]) * 0.25f);
        }
        const size_t pix = slot * hw + p0 + p;
        const int xg = x0 + 8 * bx;
        const int H1 = H >> 1, W1 = W >> 1;
        T* o1 = (T*)a.out[1] + pix * ((size_t)H1 * W1) + (xg >> 1);
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int y1 = 4 * band + r;
          if (y1 < H1) {
            T* d = o1 + (size_t)y1 * W1;
            if constexpr (HALF) *(uint2*)d = *(const uint2*)l1[r];
            else *(uint4*)d = *(const uint4*)l1[r];
          }
        }
        if (a.levels > 2) {
          T l2[2][2];
#pragma unroll
          for (int r = 0; r < 2; r++)
#pragma unroll
            for (int c = 0; c < 2; c++)
              l2[r][c] = (T)(((((float)l1[2 * r][2 * c] + (float)l1[2 * r][2 * c + 1]) + (float)l1[2 * r + 1][2 * c]) +
                              (float)l1[2 * r + 1][2 * c + 1]) * 0.25f);
          const int H2 = H >> 2, W2 = W >> 2;
          T* o2 = (T*)a.out[2] + pix * ((size_t)H2 * W2) + (xg >> 2);
#pragma unroll
          for (int r = 0; r < 2; r++) {
            const int y2 = 2 * band + r;
            if (y2 < H2) {
              T* d = o2 + (size_t)y2 * W2;
              d[0] = l2[r][0];
              d[1] = l2[r][1];
            }
          }
          if (a.levels > 3) {
            const int H3 = H >> 3, W3 = W >> 3;
            if (band < H3)
              ((T*)a.out[3])[pix * ((size_t)H3 * W3) + (size_t)band * W3 + (xg >> 3)] =
                  (T)(((((float)l2[0][0] + (float)l2[0][1]) + (float)l2[1][0]) + (float)l2[1][1]) * 0.25f);
          }
        }
      }
    }
  }
}

// Shapes the kernel takes (checked by the C entry point before any HIP call): C % 32 == 0, C <= 256, h, w >= 8,
// w % 8 == 0, h * w % 16 == 0, levels 1..4.
// slots == nullptr: edge e goes to slot slot0 + e; else to slots[e] of the cap slots (checked on the device).
int launch_corr_volume_pyramid(const void* fmaps, const int64_t* ii, const int64_t* jj, void* const* levels_out, int E,
                               int nbuf, int ncam, int C, int H, int W, int levels, long long slot0, const int64_t* slots,
                               long long cap, int dtype, hipStream_t s) {
  if (dtype != DROID_F16 && dtype != DROID_F32) return DROID_E_ARG;
  CvArgs a{};
  a.fmaps = fmaps; a.ii = ii; a.jj = jj;
  for (int l = 0; l < levels; l++) a.out[l] = levels_out[l];
  a.E = E; a.nbuf = nbuf; a.ncam = ncam; a.C = C; a.H = H; a.W = W; a.levels = levels; a.slot0 = slot0;
  a.slots = slots; a.cap = cap;
  const int P = dtype == DROID_F16 ? CvCfg<_Float16>::P : CvCfg<float>::P;
  const long long hw = (long long)H * W;
  a.nptiles = (int)((hw + P - 1) / P);
  a.nbands = (H + 7) / 8;
  a.nxc = (W + 63) / 64;
  const long long grid = (long long)E * a.nptiles;
  if (grid > 0x7fffffffLL) return DROID_E_ARG;
  if (dtype == DROID_F16)
    hipLaunchKernelGGL(corr_volume_pyramid_kernel<_Float16>, dim3((unsigned)grid), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(corr_volume_pyramid_kernel<float>, dim3((unsigned)grid), dim3(256), 0, s, a);
  return DROID_OK;
}

}  // namespace droid
