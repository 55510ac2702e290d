// launchers.hpp -- the host entry points of the kernel files that api.hip calls, grouped by the file that defines each
// one.  api.hip and every defining file include it, so a signature that drifts is a compile or link error.  (The BA,
// Cholesky-solve and proximity launchers are declared in ba_internal.hpp and graph.hpp.)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace droid {
// corr.hip
int launch_corr_index_forward(const void* volume, const float* coords, void* corr, int B, int H1,
                              int W1, int H2, int W2, int r, int dtype, hipStream_t s);
int launch_corr_pyramid_forward(const void* const* volumes, const float* coords, void* corr, int B, int H1, int W1,
                                int r, int levels, int dtype, hipStream_t s);
int launch_corr_pyramid_forward_slots(const void* const* volumes, const int64_t* slots, long long cap, const float* coords,
                                      void* corr, int B, int H1, int W1, int r, int levels, int dtype, hipStream_t s);
int launch_corr_encode(const void* const* volumes, const int64_t* slots, long long cap, const float* coords,
                       const void* packed, void* out, int B, int H1, int W1, int dtype, int hw2, hipStream_t s);
int launch_corr_index_backward(const float* coords, const void* corr_grad, void* volume_grad, int B,
                               int H1, int W1, int H2, int W2, int r, int dtype, hipStream_t s);
int launch_altcorr_pyramid_forward(const void* const* levels_dev, const int64_t* ii, const int64_t* jj,
                                   const float* coords, float* corr, int E, int frames, int H, int W, int C,
                                   int r, int nlevels, int dtype, hipStream_t s);
int launch_altcorr_forward(const void* f1, const void* f2, const float* coords, void* corr, int B,
                           int N, int H1, int W1, int H2, int W2, int C, int r, int dtype,
                           hipStream_t s);
int launch_altcorr_backward(const float* f1, const float* f2, const float* coords,
                            const float* corr_grad, float* f1g, float* f2g, int B, int N, int H1,
                            int W1, int H2, int W2, int C, int r, hipStream_t s);
// corr_volume.hip
int launch_corr_volume_pyramid(const void* fmaps, const int64_t* ii, const int64_t* jj, void* const* levels_out, int E,
                               int nbuf, int ncam, int C, int H, int W, int levels, long long slot0, const int64_t* slots,
                               long long cap, int dtype, hipStream_t s);
// geom.hip
void launch_frame_distance(const float* poses, const float* disps, const float* intr,
                           const int64_t* ii, const int64_t* jj, int E, int nbuf, int H, int W,
                           float beta, float* dist, hipStream_t s);
void launch_frame_distance_matrix(const float* poses, const float* disps, const float* intr, int n, int H, int W,
                                  float beta, float* dist, hipStream_t s);
void launch_projmap(const float* poses, const float* disps, const float* intr, const int64_t* ii,
                    const int64_t* jj, int E, int nbuf, int H, int W, float* coords, float* valid,
                    hipStream_t s);
void launch_reproject_motion(const float* poses, const float* disps, const float* intr, int intr_stride,
                             const int64_t* ii, const int64_t* jj, const float* target, int E, int nbuf, int H,
                             int W, float* coords, float* valid, float* motn, hipStream_t s);
void launch_iproj(const float* poses, const float* disps, const float* intr, int nm, int H, int W,
                  float* points, hipStream_t s);
void launch_depth_filter(const float* poses, const float* disps, const float* intr,
                         const int64_t* ix, const float* thresh, int num, int nbuf, int H, int W,
                         float* counter, hipStream_t s);
// motion_encode.hip
void launch_motion_encode(const float* poses, const float* disps, const float* intr, int intr_stride, const int64_t* ii,
                          const int64_t* jj, const float* target, const float* motn_in, const void* packed, float* coords,
                          float* valid, void* out, int E, int nbuf, int H, int W, hipStream_t s);
// heads.hip
void launch_update_heads(const void* const* x, const void* const* packed, void* const* out, const int* n_out,
                         const int* act, int heads, int B, int H, int W, hipStream_t s);
// conv3x3.hip
void launch_conv3x3(const void* x, const void* packed, void* y, int B, int c_in, int c_out, int H, int W,
                    int64_t x_batch_stride, int64_t y_batch_stride, int64_t y_group_stride, int group_channels, int relu,
                    hipStream_t s);
// gru.hip (include/droid_gru_hip.h: the arguments under their names there)
size_t gru_packed_bytes(int c_in);
size_t gru_context_workspace_bytes(int B, int H, int W);
size_t gru_workspace_bytes(int B, int H, int W);
void launch_gru_context(const void* net, int64_t net_batch_stride, const void* packed, int c_in, int B, int H, int W,
                        float* g, void* ws, hipStream_t s);
void launch_gru_gates(const void* const* seg, const int64_t* seg_batch_stride, const int* seg_channels, int nseg,
                      const void* packed, const float* g, void* z, void* rnet, int B, int H, int W, hipStream_t s);
void launch_gru_update(const void* const* seg, const int64_t* seg_batch_stride, const int* seg_channels, int nseg,
                       const void* packed, const float* g, const void* z, const void* net, int64_t net_batch_stride,
                       void* out, int64_t out_batch_stride, int B, int H, int W, hipStream_t s);
// upsample.hip
void launch_cvx_upsample(const float* data, const int64_t* ix, const void* mask, float* out, int n, int nbuf, int H, int W,
                         bool half_mask, hipStream_t s);
// graph_agg.hip
size_t graph_mean_workspace_bytes(int E, int range);
void launch_graph_mean(const void* src, const int64_t* index, void* out, int E, int64_t plane, int M, int range,
                       int compact, bool half, int* groups_out, void* workspace, hipStream_t s);
// ba_inputs.hip (include/droid_update_hip.h: the arguments of droid_ba_inputs under their names there)
struct BaInputsArgs {
  const int64_t *ii, *jj;
  const float* a;
  const void *delta, *w, *damping_net;
  float* damping_buf;
  const int64_t *ii_inac, *jj_inac;
  const float *target_inac, *weight_inac;
  int E, Ei, H, W, nbuf, n_damp;
  bool net_half, damp_half;
  int t0;
  float ep;
  float *target_state, *weight_state;
  int64_t *ii_ba, *jj_ba;
  float *target_ba, *weight_ba, *eta;
  int64_t *frames_active, *frames_eta;
  int* info;
  void* workspace;
};
size_t ba_inputs_workspace_bytes(int E, int Ei, int nbuf);
void launch_ba_inputs(const BaInputsArgs& x, hipStream_t s);
// se3_ops.hip
void launch_se3_unary(const float* in, float* out, int64_t n, int op, hipStream_t s);
void launch_se3_mul(const float* a, int stride_a, const float* b, int stride_b, float* out, int64_t n, hipStream_t s);
void launch_pose_interpolate(const float* poses, const float* tstamp, int N, const float* query, int M, float* out,
                             int64_t* k0_out, int64_t* k1_out, hipStream_t s);
// point_cloud.hip
size_t point_cloud_workspace_bytes(int n, int H, int W);
void launch_point_cloud(const float* poses, const float* disps, const float* intr, const int64_t* index,
                        const float* thresh, const uint8_t* images, int n, int nbuf, int H, int W, int min_count,
                        double disp_ratio, float* points, float* colors, int* src, int* offsets, float* matrices,
                        void* workspace, hipStream_t s);
// chol.hip
void launch_chol_pack(const double* A, const double* b, double* S, int n, int ld, hipStream_t s);
}  // namespace droid
