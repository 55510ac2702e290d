// api.hip -- the extern "C" boundary (include/droid_backends_hip.h).  Host-side only: argument
// checks, workspace carving, kernel launches on the caller's stream.  No synchronisation except
// in droid_ba_status.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include <map>
#include <mutex>

#include "../../include/droid_backends_hip.h"
#include "../../include/droid_conv3x3_hip.h"
#include "../../include/droid_gru_hip.h"
#include "../../include/droid_test_hooks_hip.h"
#include "../../include/droid_heads_hip.h"
#include "../../include/droid_motion_encode_hip.h"
#include "../../include/droid_update_hip.h"
#include "ba_internal.hpp"
#include "graph.hpp"
#include "launchers.hpp"

using namespace droid;

static thread_local char g_err[512] = "";

// workspace -> host-visible status words (droid_ba_attach_status_mirror)
static std::map<const void*, int*> g_mirror;
static std::mutex g_mirror_mu;
// workspace -> launch hints (droid_ba_attach_launch_hints) + tag of the last prepare.  Tags come from ONE counter of the
// process that attaching never resets: the words a prepare reads back may still hold the hint of an earlier prepare (of
// this buffer, or of another one the same words were attached to before: a grown workspace), possibly still in flight,
// and that hint must never carry the current tag.
struct HintState { int* ptr; int tag; };
static std::map<const void*, HintState> g_hint;
static int g_hint_tag = 0;   // guarded by g_mirror_mu
static void hints_of(BaView& v, const void* ws, bool new_call) {
  std::lock_guard<std::mutex> lock(g_mirror_mu);
  auto it = g_hint.find(ws);
  if (it == g_hint.end()) return;
  if (new_call) it->second.tag = g_hint_tag = g_hint_tag >= (1 << 30) ? 1 : g_hint_tag + 1;
  if (it->second.tag == 0) return;   // no prepare since the words were attached: nothing to expect in them
  v.hint = it->second.ptr;
  v.hint_tag = it->second.tag;
}
static int* mirror_of(const void* ws) {
  std::lock_guard<std::mutex> lock(g_mirror_mu);
  auto it = g_mirror.find(ws);
  return it == g_mirror.end() ? nullptr : it->second;
}

static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

static int fail_hip(const char* where, hipError_t e) {
  return e == hipSuccess ? DROID_OK : fail(DROID_E_HIP, "%s: %s", where, hipGetErrorString(e));
}

static int check_hip(const char* where) { return fail_hip(where, hipGetLastError()); }

// [p, p + p_bytes) and [q, q + q_bytes) share a byte.  An end beyond the address space saturates.
static bool bytes_overlap(const void* p, uint64_t p_bytes, const void* q, uint64_t q_bytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  const uintptr_t a1 = a + (p_bytes > UINTPTR_MAX - a ? UINTPTR_MAX - a : p_bytes);
  const uintptr_t b1 = b + (q_bytes > UINTPTR_MAX - b ? UINTPTR_MAX - b : q_bytes);
  return p_bytes > 0 && q_bytes > 0 && a < b1 && b < a1;
}
// bytes of `elems` floats, saturating: a record count near 2^58 times 64 bytes wraps
static uint64_t f32_bytes(uint64_t elems) { return elems > UINT64_MAX / 4 ? UINT64_MAX : elems * 4; }

static bool null_level(const void* const* levels, int n) {
  for (int l = 0; l < n; l++)
    if (!levels[l]) return true;
  return false;
}

// sizes, radius and dtype of the corr_index_* / altcorr_* entry points (N = C = 1 where an operator has none)
static int corr_check(const char* name, int B, int N, int H1, int W1, int H2, int W2, int C, int radius, int dtype) {
  if (B < 0 || N <= 0 || H1 <= 0 || W1 <= 0 || H2 <= 0 || W2 <= 0 || C <= 0 || radius < 0 || radius > 7)
    return fail(DROID_E_ARG, "%s: bad %s", name, "shape/radius");
  if (dtype < DROID_F16 || dtype > DROID_F64) return fail(DROID_E_ARG, "%s: bad %s", name, "dtype");
  return DROID_OK;
}

// The volume lookups and their gradient keep a query pixel index (H1 * W1) and the byte count of one plane (H2 * W2 * 8 for
// doubles) in 32 bits; element offsets into the volumes are 64-bit.
static int corr_map_check(const char* name, int H1, int W1, int H2, int W2) {
  if ((long long)H1 * W1 > (1ll << 27) || (long long)H2 * W2 > (1ll << 27))
    return fail(DROID_E_ARG, "%s: bad %s", name, "map size (H1 * W1 and H2 * W2 at most 2^27)");
  return DROID_OK;
}

extern "C" {

int droid_abi_version(void) { return DROID_ABI_VERSION; }
const char* droid_last_error(void) { return g_err; }

// ---------------------------------------------------------------------------- correlation
int droid_corr_index_forward(const void* volume, const float* coords, void* corr, int B, int H1,
                             int W1, int H2, int W2, int radius, int dtype, void* stream) {
  if (int rc = corr_check("corr_index_forward", B, 1, H1, W1, H2, W2, 1, radius, dtype)) return rc;
  if (int rc = corr_map_check("corr_index_forward", H1, W1, H2, W2)) return rc;
  if (B == 0) return DROID_OK;
  if (!volume || !coords || !corr) return fail(DROID_E_ARG, "corr_index_forward: null %s", "pointer");
  int rc = launch_corr_index_forward(volume, coords, corr, B, H1, W1, H2, W2, radius, dtype,
                                     (hipStream_t)stream);
  if (rc) return fail(rc, "corr_index_forward: %s", "unsupported configuration");
  return check_hip("corr_index_forward");
}

int droid_corr_pyramid_forward(const void* const* volumes, const float* coords, void* corr, int B, int H1, int W1,
                               int radius, int levels, int dtype, void* stream) {
  if (B < 0 || H1 <= 0 || W1 <= 0 || levels < 1) return fail(DROID_E_ARG, "corr_pyramid_forward: bad %s", "shape");
  if (int rc = corr_map_check("corr_pyramid_forward", H1, W1, H1, W1)) return rc;
  if (dtype < DROID_F16 || dtype > DROID_F64) return fail(DROID_E_ARG, "corr_pyramid_forward: bad %s", "dtype");
  if (B == 0) return DROID_OK;
  if (!volumes || !coords || !corr) return fail(DROID_E_ARG, "corr_pyramid_forward: null %s", "pointer");
  if (null_level(volumes, levels)) return fail(DROID_E_ARG, "corr_pyramid_forward: null %s", "pyramid level");
  int rc = launch_corr_pyramid_forward(volumes, coords, corr, B, H1, W1, radius, levels, dtype, (hipStream_t)stream);
  if (rc) return fail(rc, "corr_pyramid_forward: %s", "unsupported configuration (radius 3 or 4, levels that divide the map)");
  return check_hip("corr_pyramid_forward");
}

// droid_corr_volume_pyramid (slots == nullptr: edge e goes to slot slot0 + e) and droid_corr_volume_pyramid_slots (by_slots)
static int corr_volume_pyramid_any(const char* name, bool by_slots, const void* fmaps, const int64_t* ii, const int64_t* jj,
                                   void* const* levels_out, const int64_t* slots, int E, int nbuf, int ncam, int C, int H, int W,
                                   int levels, int64_t slot0, int64_t cap, int dtype, void* stream) {
  if (dtype != DROID_F16 && dtype != DROID_F32) return fail(DROID_E_ARG, "%s: bad %s", name, "dtype (f16 or f32)");
  if (E < 0 || nbuf <= 0 || ncam < 1 || ncam > 2) return fail(DROID_E_ARG, "%s: bad %s", name, "E / nbuf / ncam");
  if (C <= 0 || C % 32 != 0 || C > 256) return fail(DROID_E_ARG, "%s: bad %s", name, "C (a multiple of 32, at most 256)");
  if (H < 8 || W < 8 || W % 8 != 0 || ((long long)H * W) % 16 != 0 || (long long)H * W > (1 << 24))
    return fail(DROID_E_ARG, "%s: bad %s", name, "map size (H, W >= 8, W % 8 == 0, H * W % 16 == 0)");
  if (levels < 1 || levels > 4) return fail(DROID_E_ARG, "%s: bad %s", name, "levels (1 .. 4)");
  if (by_slots && cap < 1) return fail(DROID_E_ARG, "%s: bad %s", name, "cap (at least 1)");
  if (!by_slots && (slot0 < 0 || cap < 0 || slot0 + E > cap)) return fail(DROID_E_ARG, "%s: %s", name, "slot0 + E exceeds cap");
  if (E == 0) return DROID_OK;
  if (by_slots && !slots) return fail(DROID_E_ARG, "%s: null %s", name, "slots");
  if (!fmaps || !ii || !jj || !levels_out) return fail(DROID_E_ARG, "%s: null %s", name, "pointer");
  if (null_level(levels_out, levels)) return fail(DROID_E_ARG, "%s: null %s", name, "pyramid level");
  int rc = launch_corr_volume_pyramid(fmaps, ii, jj, levels_out, E, nbuf, ncam, C, H, W, levels, (long long)slot0, slots,
                                      (long long)cap, dtype, (hipStream_t)stream);
  if (rc) return fail(rc, "%s: %s", name, "unsupported configuration");
  return check_hip(name);
}

int droid_corr_volume_pyramid(const void* fmaps, const int64_t* ii, const int64_t* jj, void* const* levels_out, int E,
                              int nbuf, int ncam, int C, int H, int W, int levels, int64_t slot0, int64_t cap, int dtype,
                              void* stream) {
  return corr_volume_pyramid_any("corr_volume_pyramid", false, fmaps, ii, jj, levels_out, nullptr, E, nbuf, ncam, C, H, W,
                                 levels, slot0, cap, dtype, stream);
}

int droid_corr_pyramid_forward_slots(const void* const* volumes, const int64_t* slots, const float* coords, void* corr,
                                     int B, int64_t cap, int H1, int W1, int radius, int levels, int dtype, void* stream) {
  if (B < 0 || B > 65535 || H1 <= 0 || W1 <= 0) return fail(DROID_E_ARG, "corr_pyramid_forward_slots: bad %s", "shape");
  if (int rc = corr_map_check("corr_pyramid_forward_slots", H1, W1, H1, W1)) return rc;
  if (dtype < DROID_F16 || dtype > DROID_F64) return fail(DROID_E_ARG, "corr_pyramid_forward_slots: bad %s", "dtype");
  if (radius != 3 && radius != 4) return fail(DROID_E_ARG, "corr_pyramid_forward_slots: bad %s", "radius (3 or 4)");
  if (levels < 1 || levels > 8 || (H1 >> (levels - 1)) < 1 || (W1 >> (levels - 1)) < 1)
    return fail(DROID_E_ARG, "corr_pyramid_forward_slots: bad %s", "levels (1 .. 8, each at least one pixel)");
  if (cap < 1) return fail(DROID_E_ARG, "corr_pyramid_forward_slots: bad %s", "cap (at least 1)");
  if (B == 0) return DROID_OK;
  if (!slots) return fail(DROID_E_ARG, "corr_pyramid_forward_slots: null %s", "slots");
  if (!volumes || !coords || !corr) return fail(DROID_E_ARG, "corr_pyramid_forward_slots: null %s", "pointer");
  if (null_level(volumes, levels)) return fail(DROID_E_ARG, "corr_pyramid_forward_slots: null %s", "pyramid level");
  int rc = launch_corr_pyramid_forward_slots(volumes, slots, (long long)cap, coords, corr, B, H1, W1, radius, levels, dtype,
                                             (hipStream_t)stream);
  if (rc) return fail(rc, "corr_pyramid_forward_slots: %s", "unsupported configuration");
  return check_hip("corr_pyramid_forward_slots");
}

int droid_corr_volume_pyramid_slots(const void* fmaps, const int64_t* ii, const int64_t* jj, void* const* levels_out,
                                    const int64_t* slots, int E, int nbuf, int ncam, int C, int H, int W, int levels,
                                    int64_t cap, int dtype, void* stream) {
  return corr_volume_pyramid_any("corr_volume_pyramid_slots", true, fmaps, ii, jj, levels_out, slots, E, nbuf, ncam, C, H, W,
                                 levels, 0, cap, dtype, stream);
}

int droid_corr_index_backward(const float* coords, const void* corr_grad, void* volume_grad, int B,
                              int H1, int W1, int H2, int W2, int radius, int dtype, void* stream) {
  if (int rc = corr_check("corr_index_backward", B, 1, H1, W1, H2, W2, 1, radius, dtype)) return rc;
  if (int rc = corr_map_check("corr_index_backward", H1, W1, H2, W2)) return rc;
  if (B == 0) return DROID_OK;
  if (!coords || !corr_grad || !volume_grad) return fail(DROID_E_ARG, "corr_index_backward: null %s", "pointer");
  int rc = launch_corr_index_backward(coords, corr_grad, volume_grad, B, H1, W1, H2, W2, radius,
                                      dtype, (hipStream_t)stream);
  if (rc) return fail(rc, "corr_index_backward: %s", "unsupported configuration");
  return check_hip("corr_index_backward");
}

int droid_altcorr_forward(const void* fmap1, const void* fmap2, const float* coords, void* corr,
                          int B, int N, int H1, int W1, int H2, int W2, int C, int radius,
                          int dtype, void* stream) {
  if (int rc = corr_check("altcorr_forward", B, N, H1, W1, H2, W2, C, radius, dtype)) return rc;
  if (B == 0) return DROID_OK;
  if (!fmap1 || !fmap2 || !coords || !corr) return fail(DROID_E_ARG, "altcorr_forward: null %s", "pointer");
  int rc = launch_altcorr_forward(fmap1, fmap2, coords, corr, B, N, H1, W1, H2, W2, C, radius,
                                  dtype, (hipStream_t)stream);
  if (rc) return fail(rc, "altcorr_forward: %s", "unsupported configuration");
  return check_hip("altcorr_forward");
}

static int altcorr_pyramid_any(const void* const* pyramid, const int64_t* ii, const int64_t* jj,
                               const float* coords, float* corr, int E, int frames, int H, int W,
                               int C, int radius, int levels, int dtype, void* stream) {
  if (E < 0 || frames <= 0 || H <= 0 || W <= 0 || C <= 0 || levels < 1 || levels > 4)
    return fail(DROID_E_ARG, "altcorr_pyramid_forward: bad %s", "shape");
  if (E == 0) return DROID_OK;
  if (!pyramid || !ii || !jj || !coords || !corr) return fail(DROID_E_ARG, "altcorr_pyramid_forward: null %s", "pointer");
  if (null_level(pyramid, levels)) return fail(DROID_E_ARG, "altcorr_pyramid_forward: null %s", "pyramid level");
  int rc = launch_altcorr_pyramid_forward(pyramid, ii, jj, coords, corr, E, frames, H, W, C, radius, levels, dtype,
                                          (hipStream_t)stream);
  if (rc) return fail(rc, "altcorr_pyramid_forward: %s", "unsupported configuration (C % 16 (fp32) / 32 (fp16) == 0, C <= 128, r in {3,4})");
  return check_hip("altcorr_pyramid_forward");
}

int droid_altcorr_pyramid_forward(const float* const* pyramid, const int64_t* ii, const int64_t* jj,
                                  const float* coords, float* corr, int E, int frames, int H, int W,
                                  int C, int radius, int levels, void* stream) {
  return altcorr_pyramid_any(reinterpret_cast<const void* const*>(pyramid), ii, jj, coords, corr, E, frames, H, W, C,
                             radius, levels, DROID_F32, stream);
}

int droid_altcorr_pyramid_forward_f16(const void* const* pyramid, const int64_t* ii, const int64_t* jj,
                                      const float* coords, float* corr, int E, int frames, int H, int W,
                                      int C, int radius, int levels, void* stream) {
  return altcorr_pyramid_any(pyramid, ii, jj, coords, corr, E, frames, H, W, C, radius, levels, DROID_F16, stream);
}

int droid_altcorr_backward(const float* fmap1, const float* fmap2, const float* coords,
                           const float* corr_grad, float* fmap1_grad, float* fmap2_grad, int B,
                           int N, int H1, int W1, int H2, int W2, int C, int radius, void* stream) {
  if (int rc = corr_check("altcorr_backward", B, N, H1, W1, H2, W2, C, radius, DROID_F32)) return rc;   // fp32 only
  if (B == 0) return DROID_OK;
  if (!fmap1 || !fmap2 || !coords || !corr_grad || !fmap1_grad || !fmap2_grad)
    return fail(DROID_E_ARG, "altcorr_backward: null %s", "pointer");
  int rc = launch_altcorr_backward(fmap1, fmap2, coords, corr_grad, fmap1_grad, fmap2_grad, B, N,
                                   H1, W1, H2, W2, C, radius, (hipStream_t)stream);
  if (rc) return fail(rc, "altcorr_backward: %s", "unsupported configuration");
  return check_hip("altcorr_backward");
}

// ---------------------------------------------------------------------------- bundle adjustment
// The dimensions every BA entry point receives, filled once per entry point
struct BaDims { int E, nbuf, H, W, M, t0, t1, motion_only; };

size_t droid_ba_workspace_bytes(int E, int nbuf, int H, int W, int t0, int t1, int M) {
  BaView v;
  if (E < 0 || nbuf <= 0 || H <= 0 || W <= 0 || t1 <= t0 || M < 0) return 0;
  return ba_carve(v, nullptr, E, nbuf, H, W, t0, t1, M);
}

static int ba_view(BaView& v, void* ws, size_t ws_bytes, const BaDims& d) {
  if (d.E < 0 || d.nbuf <= 0 || d.H <= 0 || d.W <= 0) return fail(DROID_E_ARG, "ba: bad %s", "sizes");
  if (d.t0 < 0 || d.t1 <= d.t0 || d.t1 > d.nbuf) return fail(DROID_E_ARG, "ba: bad %s", "window [t0,t1)");
  if (d.M < 0 || d.M > d.nbuf) return fail(DROID_E_ARG, "ba: bad %s", "depth-slot count (eta rows)");
  // a rank of an edge-sharded call that owns no window frame and holds no edge has no depth slot: its build is zeros
  if (!d.motion_only && d.M == 0 && d.E > 0) return fail(DROID_E_ARG, "ba: %s", "eta has no rows");
  if (!ws) return fail(DROID_E_ARG, "ba: null %s", "workspace");
  const size_t need = ba_carve(v, ws, d.E, d.nbuf, d.H, d.W, d.t0, d.t1, d.motion_only ? 0 : d.M);
  if (ws_bytes < need) return fail(DROID_E_WORKSPACE, "ba: %s", "workspace too small");
  return DROID_OK;
}

int droid_ba_prepare(const int64_t* ii, const int64_t* jj, int E, int nbuf, int H, int W, int M,
                     int t0, int t1, int own0, int own1, int motion_only, void* workspace,
                     size_t workspace_bytes, void* stream) {
  BaView v;
  int rc = ba_view(v, workspace, workspace_bytes, BaDims{E, nbuf, H, W, M, t0, t1, motion_only});
  if (rc) return rc;
  if (E > 0 && (!ii || !jj)) return fail(DROID_E_ARG, "ba: null %s", "edge arrays");
  v.own0 = own0 < 0 ? 0 : own0;
  v.own1 = own1 > nbuf ? nbuf : own1;
  v.motion_only = motion_only ? 1 : 0;
  hints_of(v, workspace, true);
  launch_prep(v, ii, jj, (hipStream_t)stream);
  // overlap mode: no reduced rows of any iteration of this call are in `sys` yet (epochs start at 1)
  (void)hipMemsetAsync(v.ov_ready, 0, sizeof(int) * ((size_t)(v.n + 1 + CHOL_NB - 1) / CHOL_NB), (hipStream_t)stream);   // (>= block columns)
  return check_hip("ba_prepare");
}

}  // extern "C"
// One Gauss-Newton iteration is these two sequences of launches; the product (droid_ba_build*, droid_ba_solve_update, and
// through them droid_ba) and droid_ba_profile_iteration both enqueue it here.  between() is called after every group of
// launches: the three build stages, the factorisation, the back-substitution, the update.
template <class Between>
static void enqueue_build(const BaView& v, const float* poses, const float* disps, const float* intrinsics,
                          const float* disps_sens, const float* targets, const float* weights, const float* eta,
                          const int64_t* ii, const int64_t* jj, bool motion_only, hipStream_t s, Between between) {
  const BaLaunchPlan plan = ba_launch_plan(v);
  for (int stage = 0; stage < 3; stage++) {
    launch_build_stage(v, plan, poses, disps, intrinsics, disps_sens, targets, weights, eta, ii, jj, motion_only, stage, s);
    between();
  }
}
template <class Between>
static void enqueue_solve_update(const BaView& v, float* poses, float* disps, const float* intrinsics, const float* weights,
                                 const int64_t* ii, const int64_t* jj, float lm, float ep, bool motion_only, float* dx_out,
                                 float* dz_out, int* status_mirror, hipStream_t s, Between between) {
  const CholSystem c(v);   // launch_chol_solve (chol.hip), spelled out so that between() fits in
  if (v.E <= 0) launch_chol_preset(c, s);   // with edges, the build's assemble units have preset the solver scratch
  const bool single = launch_chol_factor(c, (double)lm, (double)ep, s);
  between();
  launch_chol_backsolve(c, single, s);
  between();
  launch_update(v, poses, disps, intrinsics, weights, ii, jj, v.xsol, dx_out, dz_out, motion_only, s, status_mirror);
  between();
}

static int ba_build_impl(const float* poses, const float* disps, const float* intrinsics,
                         const float* disps_sens, const float* targets, const float* weights,
                         const float* eta, const int64_t* ii, const int64_t* jj, const BaDims& d, void* workspace,
                         size_t workspace_bytes, void* stream, int packed) {
  BaView v;
  int rc = ba_view(v, workspace, workspace_bytes, d);
  if (rc) return rc;
  v.packed = packed;
  hints_of(v, workspace, false);
  if (!poses || !disps || !intrinsics) return fail(DROID_E_ARG, "ba: null %s", "state pointer");
  if (d.E > 0 && (!targets || !weights || !ii || !jj)) return fail(DROID_E_ARG, "ba: null %s", "edge data");
  if (!d.motion_only && d.M > 0 && (!eta || !disps_sens)) return fail(DROID_E_ARG, "ba: null %s", "eta/disps_sens");
  enqueue_build(v, poses, disps, intrinsics, disps_sens, targets, weights, eta, ii, jj, d.motion_only != 0,
                (hipStream_t)stream, [] {});
  return check_hip("ba_build");
}
extern "C" {

int droid_ba_build(const float* poses, const float* disps, const float* intrinsics,
                   const float* disps_sens, const float* targets, const float* weights,
                   const float* eta, const int64_t* ii, const int64_t* jj, int E, int nbuf, int H,
                   int W, int M, int t0, int t1, int motion_only, void* workspace,
                   size_t workspace_bytes, void* stream) {
  return ba_build_impl(poses, disps, intrinsics, disps_sens, targets, weights, eta, ii, jj,
                       BaDims{E, nbuf, H, W, M, t0, t1, motion_only}, workspace, workspace_bytes, stream, 0);
}

int droid_ba_build_packed(const float* poses, const float* disps, const float* intrinsics,
                          const float* disps_sens, const float* targets, const float* weights,
                          const float* eta, const int64_t* ii, const int64_t* jj, int E, int nbuf, int H,
                          int W, int M, int t0, int t1, int motion_only, void* workspace,
                          size_t workspace_bytes, void* stream) {
  return ba_build_impl(poses, disps, intrinsics, disps_sens, targets, weights, eta, ii, jj,
                       BaDims{E, nbuf, H, W, M, t0, t1, motion_only}, workspace, workspace_bytes, stream, 1);
}

double* droid_ba_packed_system(void* workspace, int E, int nbuf, int H, int W, int t0, int t1, int M,
                               size_t* n_elements) {
  BaView v;
  if (!workspace || t1 <= t0) return nullptr;
  ba_carve(v, workspace, E, nbuf, H, W, t0, t1, M);
  if (n_elements) *n_elements = pk_total(v.n);
  return v.psys;
}

int droid_ba_unpack_system(int E, int nbuf, int H, int W, int M, int t0, int t1, int motion_only, void* workspace,
                           size_t workspace_bytes, void* stream) {
  BaView v;
  int rc = ba_view(v, workspace, workspace_bytes, BaDims{E, nbuf, H, W, M, t0, t1, motion_only});
  if (rc) return rc;
  launch_unpack_system(v, (hipStream_t)stream);
  return check_hip("ba_unpack_system");
}

// ---- overlap of the all-reduce with the solve (multi-GPU) ------------------------------------------------------
// Chunks of the packed system by block columns of 64: 1, 1, 2, 3, 4, 5, ... block columns.  The first ones are
// small in columns (a block column on the left is the tallest: column 0 alone is 8 % of the bytes) because the
// factorisation starts on them; the later, larger chunks arrive long before the diagonal chain reaches their columns.
static int overlap_bounds(int n, int max_chunks, int* bcol /*[max_chunks + 1]*/) {
  const int nb = (n + CHOL_NB - 1) / CHOL_NB;
  int nc = 0, b = 0, size = 1, ones = 0;
  bcol[0] = 0;
  while (b < nb && nc < max_chunks) {
    b = (nc + 1 == max_chunks || b + size >= nb) ? nb : b + size;
    bcol[++nc] = b;
    if (++ones >= 2) size++;
  }
  return nc;
}

int droid_ba_overlap_plan(int t0, int t1, int max_chunks, int* nchunks_out, size_t* packed_offsets) {
  if (t1 <= t0 || max_chunks < 1 || max_chunks > 32 || !nchunks_out || !packed_offsets)
    return fail(DROID_E_ARG, "ba_overlap_plan: bad %s", "argument");
  const int n = 6 * (t1 - t0);
  int brow[33];
  const int nc = overlap_bounds(n, max_chunks, brow);
  const int nb = (n + CHOL_NB - 1) / CHOL_NB;
  for (int c = 0; c <= nc; c++) packed_offsets[c] = brow[c] >= nb ? pk_total(n) : pk_colbase(n, brow[c]);
  *nchunks_out = nc;
  return DROID_OK;
}

int droid_ba_overlap_available(int t0, int t1) {
  return (t1 > t0 && chol_overlap_available(6 * (t1 - t0))) ? 1 : 0;
}

int droid_ba_unpack_chunk(int E, int nbuf, int H, int W, int M, int t0, int t1, int chunk, int max_chunks, float lm,
                          float ep, int epoch, void* workspace, size_t workspace_bytes, void* stream) {
  BaView v;
  int rc = ba_view(v, workspace, workspace_bytes, BaDims{E, nbuf, H, W, M, t0, t1, 0});
  if (rc) return rc;
  int brow[33];
  if (max_chunks < 1 || max_chunks > 32) return fail(DROID_E_ARG, "ba_unpack_chunk: bad %s", "max_chunks");
  const int nc = overlap_bounds(v.n, max_chunks, brow);
  if (chunk < 0 || chunk >= nc || epoch <= 0) return fail(DROID_E_ARG, "ba_unpack_chunk: bad %s", "chunk / epoch");
  launch_unpack_cols(v, brow[chunk], brow[chunk + 1], (double)lm, (double)ep, epoch, (hipStream_t)stream);
  return check_hip("ba_unpack_chunk");
}

// the pointers droid_ba_solve_update and droid_ba_solve_update_overlap read
static int solve_update_check(const float* poses, const float* disps, const float* intrinsics, const float* weights,
                              const int64_t* ii, const int64_t* jj, int E, int motion_only) {
  if (!poses || !disps) return fail(DROID_E_ARG, "ba: null %s", "state pointer");
  if (!motion_only && (!intrinsics || (E > 0 && (!weights || !ii || !jj))))
    return fail(DROID_E_ARG, "ba: null %s", "intrinsics/weights/edges");
  return DROID_OK;
}

int droid_ba_solve_update_overlap(float* poses, float* disps, const float* intrinsics, const float* weights,
                                  const int64_t* ii, const int64_t* jj, int E, int nbuf, int H, int W, int M,
                                  int t0, int t1, int epoch, int motion_only, float* dx_out, float* dz_out,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  BaView v;
  int rc = ba_view(v, workspace, workspace_bytes, BaDims{E, nbuf, H, W, M, t0, t1, motion_only});
  if (!rc) rc = solve_update_check(poses, disps, intrinsics, weights, ii, jj, E, motion_only);
  if (rc) return rc;
  if (E <= 0 || epoch <= 0) return fail(DROID_E_ARG, "ba_solve_update_overlap: needs %s", "edges (the build presets the solver scratch) and epoch > 0");
  hipStream_t s = (hipStream_t)stream;
  const CholSystem c(v);
  if (!launch_chol_factor_overlap(c, v.ov_ready, epoch, s))
    return fail(DROID_E_ARG, "ba_solve_update_overlap: %s", "the single-launch solver is not available for this system (unpack and call droid_ba_solve_update)");
  launch_chol_backsolve(c, true, s);
  launch_update(v, poses, disps, intrinsics, weights, ii, jj, v.xsol, dx_out, dz_out, motion_only != 0, s,
                mirror_of(workspace));
  return check_hip("ba_solve_update_overlap");
}

int droid_ba_solve_update(float* poses, float* disps, const float* intrinsics, const float* weights,
                          const int64_t* ii, const int64_t* jj, int E, int nbuf, int H, int W, int M,
                          int t0, int t1, float lm, float ep, int motion_only, float* dx_out,
                          float* dz_out, void* workspace, size_t workspace_bytes, void* stream) {
  BaView v;
  int rc = ba_view(v, workspace, workspace_bytes, BaDims{E, nbuf, H, W, M, t0, t1, motion_only});
  if (!rc) rc = solve_update_check(poses, disps, intrinsics, weights, ii, jj, E, motion_only);
  if (rc) return rc;
  enqueue_solve_update(v, poses, disps, intrinsics, weights, ii, jj, lm, ep, motion_only != 0, dx_out, dz_out,
                       mirror_of(workspace), (hipStream_t)stream, [] {});
  return check_hip("ba_solve_update");
}

int droid_ba(float* poses, float* disps, const float* intrinsics, const float* disps_sens,
             const float* targets, const float* weights, const float* eta, const int64_t* ii,
             const int64_t* jj, int E, int nbuf, int H, int W, int M, int t0, int t1,
             int iterations, float lm, float ep, int motion_only, float* dx_out, float* dz_out,
             void* workspace, size_t workspace_bytes, void* stream) {
  // one rank owns the whole window (t1 > t0): there is at least one depth slot
  if (!motion_only && M == 0 && t1 > t0) return fail(DROID_E_ARG, "ba: %s", "eta has no rows");
  int rc = droid_ba_prepare(ii, jj, E, nbuf, H, W, M, t0, t1, 0, nbuf, motion_only, workspace,
                            workspace_bytes, stream);
  if (rc) return rc;
  for (int it = 0; it < iterations; it++) {
    rc = droid_ba_build(poses, disps, intrinsics, disps_sens, targets, weights, eta, ii, jj, E,
                        nbuf, H, W, M, t0, t1, motion_only, workspace, workspace_bytes, stream);
    if (rc) return rc;
    rc = droid_ba_solve_update(poses, disps, intrinsics, weights, ii, jj, E, nbuf, H, W, M, t0, t1, lm, ep, motion_only,
                               dx_out, dz_out, workspace, workspace_bytes, stream);
    if (rc) return rc;
  }
  return DROID_OK;
}

// Measurement support: one Gauss-Newton iteration (after droid_ba_prepare) with a HIP event
// between kernel groups on `stream`; blocks until done.  stage_ms[8] = {memset+linearise,
// assemble, fused E-rows + Schur SYRK + rhs, (unused: 0), damp+factor, back-substitution solve, dx/disps/poses update, total}.
int droid_ba_profile_iteration(float* poses, float* disps, const float* intrinsics,
                               const float* disps_sens, const float* targets, const float* weights,
                               const float* eta, const int64_t* ii, const int64_t* jj, int E,
                               int nbuf, int H, int W, int M, int t0, int t1, float lm, float ep,
                               int motion_only, void* workspace, size_t workspace_bytes,
                               void* stream, float* stage_ms) {
  BaView v;
  int rc = ba_view(v, workspace, workspace_bytes, BaDims{E, nbuf, H, W, M, t0, t1, motion_only});
  if (rc) return rc;
  hints_of(v, workspace, false);
  if (!stage_ms) return fail(DROID_E_ARG, "ba_profile: null %s", "stage_ms");
  hipStream_t s = (hipStream_t)stream;
  hipEvent_t ev[7];
  for (auto& e : ev) (void)hipEventCreate(&e);
  int nev = 0;
  auto record = [&] { (void)hipEventRecord(ev[nev++], s); };
  record();
  // the product's iteration, without outputs and without a status mirror
  enqueue_build(v, poses, disps, intrinsics, disps_sens, targets, weights, eta, ii, jj, motion_only != 0, s, record);
  enqueue_solve_update(v, poses, disps, intrinsics, weights, ii, jj, lm, ep, motion_only != 0, nullptr, nullptr, nullptr, s,
                       record);
  hipError_t e = hipEventSynchronize(ev[6]);
  stage_ms[3] = 0.0f;
  for (int k = 0; k < 6; k++) (void)hipEventElapsedTime(&stage_ms[k < 3 ? k : k + 1], ev[k], ev[k + 1]);
  (void)hipEventElapsedTime(&stage_ms[7], ev[0], ev[6]);
  for (auto& x : ev) (void)hipEventDestroy(x);
  if (e != hipSuccess) return fail_hip("ba_profile", e);
  return check_hip("ba_profile_iteration");
}

double* droid_ba_system(void* workspace, int E, int nbuf, int H, int W, int t0, int t1, int M,
                        size_t* n_elements) {
  BaView v;
  if (!workspace || t1 <= t0) return nullptr;
  ba_carve(v, workspace, E, nbuf, H, W, t0, t1, M);
  if (n_elements) *n_elements = (size_t)(v.n + 1) * v.ld;
  return v.sys;
}

int droid_ba_status(const void* workspace, void* stream, int* status_out, int* depth_slots_out) {
  if (!workspace) return fail(DROID_E_ARG, "ba_status: null %s", "workspace");
  int hdr[HDR_WORDS];
  hipError_t e = hipMemcpyAsync(hdr, workspace, sizeof(hdr), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) return fail_hip("ba_status", e);
  if (status_out) *status_out = hdr[HDR_STATUS];
  if (depth_slots_out) *depth_slots_out = hdr[HDR_M];
  return DROID_OK;
}

int droid_ba_attach_launch_hints(const void* workspace, int* hints) {
  if (!workspace) return fail(DROID_E_ARG, "ba_attach_launch_hints: null %s", "workspace");
  std::lock_guard<std::mutex> lock(g_mirror_mu);
  if (hints) {
    hints[0] = hints[1] = 0;   // tag 0 is never a prepare's
    g_hint[workspace] = HintState{hints, 0};
  }
  else g_hint.erase(workspace);
  return DROID_OK;
}

int droid_ba_attach_status_mirror(const void* workspace, int* mirror) {
  if (!workspace) return fail(DROID_E_ARG, "ba_attach_status_mirror: null %s", "workspace");
  std::lock_guard<std::mutex> lock(g_mirror_mu);
  if (mirror) g_mirror[workspace] = mirror;
  else g_mirror.erase(workspace);
  return DROID_OK;
}

int droid_test_wave_reduce32(const float* in, float* out, void* stream) {
  if (!in || !out) return fail(DROID_E_ARG, "test_wave_reduce32: null %s", "pointer");
  launch_wave_reduce32_test(in, out, (hipStream_t)stream);
  return check_hip("test_wave_reduce32");
}

int droid_test_ba_lin(const float* poses, const float* disps, const float* intrinsics, const float* disps_sens,
                      const float* targets, const float* weights, const float* eta, const int64_t* ii, const int64_t* jj,
                      int E, int nbuf, int H, int W, int M, int t0, int t1, int motion_only, int ragged, void* workspace,
                      size_t workspace_bytes, float* hpart_out, float* q_out, float* w_out, float* ebuf_out,
                      size_t* words_out, void* stream) {
  const BaDims d{E, nbuf, H, W, M, t0, t1, motion_only};
  BaView v;
  if (int rc = ba_view(v, workspace, workspace_bytes, d)) return rc;
  if (!poses || !disps || !intrinsics) return fail(DROID_E_ARG, "test_ba_lin: null %s", "state pointer");
  if (E > 0 && (!targets || !weights || !ii || !jj)) return fail(DROID_E_ARG, "test_ba_lin: null %s", "edge data");
  if (!motion_only && v.M > 0 && (!eta || !disps_sens)) return fail(DROID_E_ARG, "test_ba_lin: null %s", "eta/disps_sens");
  hipStream_t s = (hipStream_t)stream;
  const size_t words[4] = {(size_t)E * v.nch * LIN_WAVES * 32, (size_t)v.M * v.HW, (size_t)v.M * v.HW,
                           v.wide ? 6 * ((size_t)v.M + E) * v.HW : 0};
  const float* src[4] = {v.Hpart, v.Q, v.w, v.Ebuf};
  float* dst[4] = {hpart_out, q_out, w_out, ebuf_out};
  if (dst[0] || dst[1] || dst[2] || dst[3])   // (no output buffer: a size query, nothing is launched)
    launch_lin_test(v, poses, disps, intrinsics, disps_sens, targets, weights, eta, ii, jj, motion_only != 0, ragged != 0, s);
  if (words_out) {   // and the host's choice of instantiation (ba_carve)
    words_out[4] = (size_t)v.wide;
    words_out[5] = (size_t)v.zsplit;
  }
  for (int k = 0; k < 4; k++) {
    if (words_out) words_out[k] = words[k];
    if (dst[k] && words[k])
      (void)hipMemcpyAsync(dst[k], src[k], sizeof(float) * words[k], hipMemcpyDeviceToDevice, s);
  }
  return check_hip("test_ba_lin");
}

size_t droid_chol_scratch_doubles(int n) { return CholSystem::scratch_doubles(n); }

int droid_chol_solve(const double* A, const double* b, double* x, int n, double* scratch,
                     int* fail_flag, void* stream) {
  if (n <= 0 || !A || !b || !x || !scratch || !fail_flag) return fail(DROID_E_ARG, "chol_solve: bad %s", "argument");
  hipStream_t s = (hipStream_t)stream;
  const CholSystem c(scratch, n, x, fail_flag);
  launch_chol_pack(A, b, c.S, c.n, c.ld, s);
  launch_chol_solve(c, 0.0, 0.0, s, false);
  return check_hip("chol_solve");
}

// ---------------------------------------------------------------------------- geometry
int droid_frame_distance(const float* poses, const float* disps, const float* intrinsics,
                         const int64_t* ii, const int64_t* jj, int E, int nbuf, int H, int W,
                         float beta, float* dist, void* stream) {
  if (E < 0 || nbuf <= 0 || H <= 0 || W <= 0) return fail(DROID_E_ARG, "frame_distance: bad %s", "sizes");
  if (E == 0) return DROID_OK;
  if (!poses || !disps || !intrinsics || !ii || !jj || !dist) return fail(DROID_E_ARG, "frame_distance: null %s", "pointer");
  launch_frame_distance(poses, disps, intrinsics, ii, jj, E, nbuf, H, W, beta, dist, (hipStream_t)stream);
  return check_hip("frame_distance");
}

int droid_frame_distance_matrix(const float* poses, const float* disps, const float* intrinsics, int n, int nbuf,
                                int H, int W, float beta, float* dist, void* stream) {
  if (n < 0 || nbuf <= 0 || n > nbuf || H <= 0 || W <= 0) return fail(DROID_E_ARG, "frame_distance_matrix: bad %s", "sizes");
  if (n == 0) return DROID_OK;
  if (!poses || !disps || !intrinsics || !dist) return fail(DROID_E_ARG, "frame_distance_matrix: null %s", "pointer");
  launch_frame_distance_matrix(poses, disps, intrinsics, n, H, W, beta, dist, (hipStream_t)stream);
  return check_hip("frame_distance_matrix");
}

int droid_projmap(const float* poses, const float* disps, const float* intrinsics,
                  const int64_t* ii, const int64_t* jj, int E, int nbuf, int H, int W,
                  float* coords, float* valid, void* stream) {
  if (E < 0 || nbuf <= 0 || H <= 0 || W <= 0) return fail(DROID_E_ARG, "projmap: bad %s", "sizes");
  if (E == 0) return DROID_OK;
  if (!poses || !disps || !intrinsics || !ii || !jj || !coords || !valid) return fail(DROID_E_ARG, "projmap: null %s", "pointer");
  launch_projmap(poses, disps, intrinsics, ii, jj, E, nbuf, H, W, coords, valid, (hipStream_t)stream);
  return check_hip("projmap");
}

int droid_reproject_motion(const float* poses, const float* disps, const float* intrinsics, int intr_stride,
                           const int64_t* ii, const int64_t* jj, const float* target, int E, int nbuf, int H, int W,
                           float* coords, float* valid, float* motn, void* stream) {
  if (E < 0 || nbuf <= 0 || H <= 0 || W <= 0 || (intr_stride != 0 && intr_stride != 4))
    return fail(DROID_E_ARG, "reproject_motion: bad %s", "sizes");
  if (E == 0) return DROID_OK;
  if (!poses || !disps || !intrinsics || !ii || !jj || !coords || !valid) return fail(DROID_E_ARG, "reproject_motion: null %s", "pointer");
  if (motn && !target) return fail(DROID_E_ARG, "reproject_motion: motn needs %s", "target");
  launch_reproject_motion(poses, disps, intrinsics, intr_stride, ii, jj, target, E, nbuf, H, W, coords, valid, motn,
                          (hipStream_t)stream);
  return check_hip("reproject_motion");
}

int droid_iproj(const float* poses, const float* disps, const float* intrinsics, int nm, int H,
                int W, float* points, void* stream) {
  if (nm < 0 || H <= 0 || W <= 0) return fail(DROID_E_ARG, "iproj: bad %s", "sizes");
  if (nm == 0) return DROID_OK;
  if (!poses || !disps || !intrinsics || !points) return fail(DROID_E_ARG, "iproj: null %s", "pointer");
  launch_iproj(poses, disps, intrinsics, nm, H, W, points, (hipStream_t)stream);
  return check_hip("iproj");
}

int droid_depth_filter(const float* poses, const float* disps, const float* intrinsics,
                       const int64_t* ix, const float* thresh, int num, int nbuf, int H, int W,
                       float* counter, void* stream) {
  if (num < 0 || nbuf <= 0 || H <= 0 || W <= 0) return fail(DROID_E_ARG, "depth_filter: bad %s", "sizes");
  if (num == 0) return DROID_OK;
  if (!poses || !disps || !intrinsics || !ix || !thresh || !counter) return fail(DROID_E_ARG, "depth_filter: null %s", "pointer");
  launch_depth_filter(poses, disps, intrinsics, ix, thresh, num, nbuf, H, W, counter, (hipStream_t)stream);
  return check_hip("depth_filter");
}

// ---------------------------------------------------------------------------- convex upsampling
int droid_cvx_upsample(const float* data, const int64_t* ix, const void* mask, float* out, int n, int nbuf_in,
                       int nbuf_out, int H, int W, int mask_dtype, void* stream) {
  if (mask_dtype != DROID_F16 && mask_dtype != DROID_F32) return fail(DROID_E_ARG, "cvx_upsample: bad %s", "mask dtype (f16 or f32)");
  if (H < 1 || W < 1) return fail(DROID_E_ARG, "cvx_upsample: bad %s", "map size (H, W >= 1)");
  if (n < 0) return fail(DROID_E_ARG, "cvx_upsample: bad %s", "n (negative)");
  if (nbuf_in < 1 || nbuf_out < 1) return fail(DROID_E_ARG, "cvx_upsample: bad %s", "nbuf_in / nbuf_out (at least 1)");
  // the kernel keeps a coarse pixel index in 32 bits and element offsets in 64
  const unsigned __int128 hw = (unsigned __int128)H * W, lim = (unsigned __int128)1 << 62;
  if (hw > 0x7fffffffu - 64 || 64 * hw * nbuf_out > lim || 576 * hw * (n > 0 ? n : 1) > lim)
    return fail(DROID_E_ARG, "cvx_upsample: %s", "8H * 8W * nbuf_out (or the mask) exceeds the kernel's index range");
  if (n == 0) return DROID_OK;
  if (!data || !mask || !out) return fail(DROID_E_ARG, "cvx_upsample: null %s", "pointer");
  launch_cvx_upsample(data, ix, mask, out, n, nbuf_in < nbuf_out ? nbuf_in : nbuf_out, H, W, mask_dtype == DROID_F16,
                      (hipStream_t)stream);
  return check_hip("cvx_upsample");
}

// ---------------------------------------------------------------------------- factor-graph edge selection
// ------------------------------------------------------------------ graph aggregation
// sizes droid_graph_mean and its workspace query check; <0 after fail()
static int graph_mean_check(int E, int range) {
  if (E < 0 || E > 65535) return fail(DROID_E_ARG, "graph_mean: bad %s", "E (0 .. 65535)");
  if (range < 1 || range > DROID_GRAPH_MEAN_MAX_RANGE)
    return fail(DROID_E_ARG, "graph_mean: bad %s", "range (1 .. 16384: the prepare step's tables live in LDS)");
  return 0;
}

size_t droid_graph_mean_workspace_bytes(int E, int range) {
  if (graph_mean_check(E, range)) return 0;
  return graph_mean_workspace_bytes(E, range);
}

int droid_graph_mean(const void* src, const int64_t* index, void* out, int E, int64_t plane, int M, int range,
                     int compact, int dtype, int* groups_out, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = graph_mean_check(E, range);
  if (rc) return rc;
  if (M < 1) return fail(DROID_E_ARG, "graph_mean: bad %s", "M (at least 1)");
  if (compact != 0 && compact != 1) return fail(DROID_E_ARG, "graph_mean: bad %s", "compact (0 or 1)");
  if (!compact && range != M) return fail(DROID_E_ARG, "graph_mean: %s", "dense mode (compact = 0) needs range == M");
  if (plane < 1) return fail(DROID_E_ARG, "graph_mean: bad %s", "plane (at least 1)");
  const int64_t lim = (int64_t)1 << 62;
  if (plane > lim / M || (E > 0 && plane > lim / E))
    return fail(DROID_E_ARG, "graph_mean: %s", "M * plane or E * plane exceeds the kernel's index range (2^62)");
  if (dtype != DROID_F16 && dtype != DROID_F32) return fail(DROID_E_ARG, "graph_mean: bad %s", "dtype (f16 or f32)");
  if (!out) return fail(DROID_E_ARG, "graph_mean: null %s", "pointer (out)");
  if (E > 0 && (!src || !index)) return fail(DROID_E_ARG, "graph_mean: null %s", "pointer (src / index)");
  hipStream_t s = (hipStream_t)stream;
  if (E == 0) {   // every row is empty: no lists to build, no workspace needed
    (void)hipMemsetAsync(out, 0, (size_t)M * (size_t)plane * (dtype == DROID_F16 ? 2 : 4), s);
    if (groups_out) (void)hipMemsetAsync(groups_out, 0, sizeof(int), s);
    return check_hip("graph_mean");
  }
  if (!workspace) return fail(DROID_E_ARG, "graph_mean: null %s", "workspace");
  if (workspace_bytes < graph_mean_workspace_bytes(E, range))
    return fail(DROID_E_WORKSPACE, "graph_mean: %s", "workspace too small");
  if ((uintptr_t)workspace % 4 != 0) return fail(DROID_E_ARG, "graph_mean: %s", "workspace is not 4-byte aligned");
  launch_graph_mean(src, index, out, E, plane, M, range, compact, dtype == DROID_F16, groups_out, workspace, s);
  return check_hip("graph_mean");
}

// sizes every proximity entry point checks; <0 after fail()
static int proximity_check(int t, int t0, int t1, int n_known, int cap) {
  if (t < 0 || t0 < 0 || t1 < 0) return fail(DROID_E_ARG, "proximity_edges: negative %s", "t / t0 / t1");
  if (t1 > t0) return fail(DROID_E_ARG, "proximity_edges: %s", "t1 > t0 (columns must start at or before the rows)");
  if (n_known < 0 || cap < 0) return fail(DROID_E_ARG, "proximity_edges: negative %s", "n_known / cap");
  if (t > t0 && (int64_t)(t - t0) * (t - t1) > PROX_MAX_CELLS)
    return fail(DROID_E_ARG, "proximity_edges: %s", "rectangle above 1048576 cells (its suppression bitmap has to fit in LDS)");
  return DROID_OK;
}

size_t droid_proximity_workspace_bytes(int t, int t0, int t1, int n_known, int cap) {
  if (proximity_check(t, t0, t1, n_known, cap)) return 0;
  return prox_workspace_bytes(t, t0, t1, n_known, cap);
}

int droid_proximity_edges(const float* dist, int ld, int bidirectional, int t, int t0, int t1, int rad, int nms,
                          float thresh, int max_factors, int stereo, const int64_t* sup_ii, const int64_t* sup_jj,
                          int n_sup, const int64_t* known_ii, const int64_t* known_jj, int n_known,
                          int64_t* edges_out, int cap, int* count_out, void* workspace, size_t workspace_bytes,
                          void* stream) {
  int rc = proximity_check(t, t0, t1, n_known, cap);
  if (rc) return rc;
  if (rad < 0) return fail(DROID_E_ARG, "proximity_edges: bad %s", "rad (< 0)");
  if (nms < 0 || nms > 1024) return fail(DROID_E_ARG, "proximity_edges: bad %s", "nms (0 .. 1024)");
  if (n_sup < 0) return fail(DROID_E_ARG, "proximity_edges: negative %s", "n_sup");
  if (ld < t) return fail(DROID_E_ARG, "proximity_edges: %s", "row pitch of dist below t");
  const int64_t bound = prox_edge_bound(t, t0, t1, rad, max_factors, stereo);
  if (cap < bound) return fail(DROID_E_ARG, "proximity_edges: %s", "cap below max(forced edges, max_factors + 2)");
  if (!count_out) return fail(DROID_E_ARG, "proximity_edges: null %s", "count_out");
  if (t > t0) {
    if (!dist || !workspace || (bound > 0 && !edges_out)) return fail(DROID_E_ARG, "proximity_edges: null %s", "dist / edges_out / workspace");
    if ((n_sup > 0 && (!sup_ii || !sup_jj)) || (n_known > 0 && (!known_ii || !known_jj)))
      return fail(DROID_E_ARG, "proximity_edges: null %s", "edge list");
    if (workspace_bytes < prox_workspace_bytes(t, t0, t1, n_known, cap))
      return fail(DROID_E_WORKSPACE, "proximity_edges: %s", "workspace too small");
  }
  ProxArgs a{dist, ld, bidirectional ? 1 : 0, t, t0, t1, rad, nms, thresh, max_factors, stereo ? 1 : 0, sup_ii, sup_jj, n_sup,
             known_ii, known_jj, n_known, edges_out, cap, count_out, workspace};
  launch_proximity_edges(a, (hipStream_t)stream);
  return check_hip("proximity_edges");
}

// ---- pose algebra (se3_ops.hip) ---------------------------------------------------------------------------------
int droid_se3_unary(const float* in, float* out, int64_t n, int op, void* stream) {
  if (op < DROID_SE3_INV || op > DROID_SE3_MATRIX) return fail(DROID_E_ARG, "se3_unary: bad %s", "op (0 .. 3)");
  if (n < 0) return fail(DROID_E_ARG, "se3_unary: bad %s", "n (negative)");
  if (n > ((int64_t)1 << 62) / 16) return fail(DROID_E_ARG, "se3_unary: %s", "n * 16 exceeds the kernel's index range (2^62)");
  if (n == 0) return DROID_OK;
  if (!in || !out) return fail(DROID_E_ARG, "se3_unary: null %s", "pointer (in / out)");
  const int win = op == DROID_SE3_EXP ? 6 : 7;
  const int wout = op == DROID_SE3_LOG ? 6 : op == DROID_SE3_MATRIX ? 16 : 7;
  if (!(op == DROID_SE3_INV && in == out) && bytes_overlap(in, f32_bytes((uint64_t)n * win), out, f32_bytes((uint64_t)n * wout)))
    return fail(DROID_E_ARG, "se3_unary: %s", "out overlaps in (only INV may run in place, with out == in)");
  launch_se3_unary(in, out, n, op, (hipStream_t)stream);
  return check_hip("se3_unary");
}

int droid_se3_mul(const float* a, int stride_a, const float* b, int stride_b, float* out, int64_t n, void* stream) {
  if (stride_a != 0 && stride_a != 7) return fail(DROID_E_ARG, "se3_mul: bad %s", "stride_a (0 or 7)");
  if (stride_b != 0 && stride_b != 7) return fail(DROID_E_ARG, "se3_mul: bad %s", "stride_b (0 or 7)");
  if (n < 0) return fail(DROID_E_ARG, "se3_mul: bad %s", "n (negative)");
  if (n > ((int64_t)1 << 62) / 16) return fail(DROID_E_ARG, "se3_mul: %s", "n * 16 exceeds the kernel's index range (2^62)");
  if (n == 0) return DROID_OK;
  if (!a || !b || !out) return fail(DROID_E_ARG, "se3_mul: null %s", "pointer (a / b / out)");
  if (!(stride_a == 7 && a == out) && bytes_overlap(a, stride_a ? (uint64_t)n * 28 : 28, out, (uint64_t)n * 28))
    return fail(DROID_E_ARG, "se3_mul: %s", "out overlaps a (allowed: out == a with stride_a = 7)");
  if (!(stride_b == 7 && b == out) && bytes_overlap(b, stride_b ? (uint64_t)n * 28 : 28, out, (uint64_t)n * 28))
    return fail(DROID_E_ARG, "se3_mul: %s", "out overlaps b (allowed: out == b with stride_b = 7)");
  launch_se3_mul(a, stride_a, b, stride_b, out, n, (hipStream_t)stream);
  return check_hip("se3_mul");
}

int droid_pose_interpolate(const float* poses, const float* tstamp, int N, const float* query, int M, float* out,
                           int64_t* k0_out, int64_t* k1_out, void* stream) {
  if (N < 1) return fail(DROID_E_ARG, "pose_interpolate: bad %s", "N (at least 1)");
  if (M < 0) return fail(DROID_E_ARG, "pose_interpolate: bad %s", "M (negative)");
  if (M == 0) return DROID_OK;
  if (!poses || !tstamp || !query || !out) return fail(DROID_E_ARG, "pose_interpolate: null %s", "pointer (poses / tstamp / query / out)");
  const struct { const void* p; uint64_t bytes; const char* name; } outs[3] = {
      {out, (uint64_t)M * 28, "out"}, {k0_out, (uint64_t)M * 8, "k0_out"}, {k1_out, (uint64_t)M * 8, "k1_out"}};
  for (const auto& o : outs) {
    if (!o.p) continue;
    if (bytes_overlap(poses, (uint64_t)N * 28, o.p, o.bytes) || bytes_overlap(tstamp, (uint64_t)N * 4, o.p, o.bytes) ||
        bytes_overlap(query, (uint64_t)M * 4, o.p, o.bytes))
      return fail(DROID_E_ARG, "pose_interpolate: %s overlaps an input (poses / tstamp / query)", o.name);
  }
  launch_pose_interpolate(poses, tstamp, N, query, M, out, k0_out, k1_out, (hipStream_t)stream);
  return check_hip("pose_interpolate");
}

// ---- point cloud (point_cloud.hip) ------------------------------------------------------------------------------
// sizes droid_point_cloud and its workspace query check; <0 after fail()
static int point_cloud_check(int n, int H, int W) {
  if (n < 0) return fail(DROID_E_ARG, "point_cloud: bad %s", "n (negative)");
  if (H < 1 || W < 1) return fail(DROID_E_ARG, "point_cloud: bad %s", "map size (H, W >= 1)");
  if ((unsigned __int128)(n > 0 ? n : 1) * (unsigned)H * (unsigned)W >= ((unsigned __int128)1 << 31))
    return fail(DROID_E_ARG, "point_cloud: %s", "n * H * W reaches 2^31 (rows and offsets are 32-bit)");
  return 0;
}

size_t droid_point_cloud_workspace_bytes(int n, int H, int W) {
  if (point_cloud_check(n, H, W)) return 0;
  return point_cloud_workspace_bytes(n, H, W);
}

int droid_point_cloud(const float* poses, const float* disps, const float* intrinsics, const int64_t* index,
                      const float* thresh, const uint8_t* images, int n, int nbuf, int H, int W, int min_count,
                      double disp_ratio, float* points, float* colors, int* src, int* offsets, float* matrices,
                      void* workspace, size_t workspace_bytes, void* stream) {
  int rc = point_cloud_check(n, H, W);
  if (rc) return rc;
  if (nbuf < 1) return fail(DROID_E_ARG, "point_cloud: bad %s", "nbuf (at least 1)");
  if (n == 0) return DROID_OK;
  if (!poses || !disps || !intrinsics || !index || !thresh)
    return fail(DROID_E_ARG, "point_cloud: null %s", "pointer (poses / disps / intrinsics / index / thresh)");
  if (!points || !src || !offsets || !matrices)
    return fail(DROID_E_ARG, "point_cloud: null %s", "pointer (points / src / offsets / matrices)");
  if ((images == nullptr) != (colors == nullptr))
    return fail(DROID_E_ARG, "point_cloud: %s", "images and colors go together (both or neither)");
  if (!workspace) return fail(DROID_E_ARG, "point_cloud: null %s", "workspace");
  if (workspace_bytes < point_cloud_workspace_bytes(n, H, W)) return fail(DROID_E_ARG, "point_cloud: %s", "workspace too small");
  if ((uintptr_t)workspace % 8 != 0) return fail(DROID_E_ARG, "point_cloud: %s", "workspace is not 8-byte aligned");
  const uint64_t hw = (uint64_t)H * W, cap = (uint64_t)n * hw;
  struct Range { const void* p; uint64_t bytes; const char* name; };
  const Range ins[6] = {{poses, (uint64_t)nbuf * 28, "poses"}, {disps, (uint64_t)nbuf * hw * 4, "disps"},
                        {intrinsics, 16, "intrinsics"}, {index, (uint64_t)n * 8, "index"}, {thresh, (uint64_t)n * 4, "thresh"},
                        {images, images ? (uint64_t)nbuf * 192 * hw : 0, "images"}};
  const Range outs[6] = {{points, cap * 12, "points"}, {colors, colors ? cap * 12 : 0, "colors"}, {src, cap * 4, "src"},
                         {offsets, ((uint64_t)n + 1) * 4, "offsets"}, {matrices, (uint64_t)n * 64, "matrices"},
                         {workspace, point_cloud_workspace_bytes(n, H, W), "workspace"}};
  for (int o = 0; o < 6; o++) {
    const Range& out = outs[o];
    for (const Range& in : ins)
      if (bytes_overlap(out.p, out.bytes, in.p, in.bytes)) return fail(DROID_E_ARG, "point_cloud: %s overlaps %s", out.name, in.name);
    for (int q = 0; q < o; q++)
      if (bytes_overlap(out.p, out.bytes, outs[q].p, outs[q].bytes))
        return fail(DROID_E_ARG, "point_cloud: %s overlaps %s", out.name, outs[q].name);
  }
  launch_point_cloud(poses, disps, intrinsics, index, thresh, images, n, nbuf, H, W, min_count, disp_ratio, points, colors,
                     src, offsets, matrices, workspace, (hipStream_t)stream);
  return check_hip("point_cloud");
}


// ---- the BA inputs of a factor-graph update (ba_inputs.hip, include/droid_update_hip.h) -------------------------
// sizes droid_ba_inputs and its workspace query check; <0 after fail()
static int ba_inputs_check(int E, int Ei, int nbuf) {
  if (E < 1) return fail(DROID_E_ARG, "ba_inputs: bad %s", "E (at least 1)");
  if (Ei < 0) return fail(DROID_E_ARG, "ba_inputs: bad %s", "Ei (negative)");
  if ((int64_t)E + Ei > 65535) return fail(DROID_E_ARG, "ba_inputs: bad %s", "E + Ei (at most 65535)");
  if (nbuf < 1 || nbuf > DROID_BA_INPUTS_MAX_NBUF)
    return fail(DROID_E_ARG, "ba_inputs: bad %s", "nbuf (1 .. 16384: the prepare launch's tables live in LDS)");
  return 0;
}

size_t droid_ba_inputs_workspace_bytes(int E, int Ei, int nbuf) {
  if (ba_inputs_check(E, Ei, nbuf)) return 0;
  return ba_inputs_workspace_bytes(E, Ei, nbuf);
}

int droid_ba_inputs(const int64_t* ii, const int64_t* jj, const float* a, const void* delta, const void* w,
                    const void* damping_net, float* damping_buf, const int64_t* ii_inac, const int64_t* jj_inac,
                    const float* target_inac, const float* weight_inac, int E, int Ei, int H, int W, int nbuf,
                    int n_damp, int net_dtype, int damp_dtype, int t0, float ep, float* target_state,
                    float* weight_state, int64_t* ii_ba, int64_t* jj_ba, float* target_ba, float* weight_ba, int cap_e,
                    float* eta, int64_t* frames_active, int64_t* frames_eta, int cap_m, int* info, void* workspace,
                    size_t workspace_bytes, void* stream) {
  int rc = ba_inputs_check(E, Ei, nbuf);
  if (rc) return rc;
  if (H < 1 || W < 1) return fail(DROID_E_ARG, "ba_inputs: bad %s", "map size (H, W >= 1)");
  const unsigned __int128 hw = (unsigned __int128)H * W, lim = (unsigned __int128)1 << 62;
  if ((unsigned)(E + Ei) * hw * 2 > lim)
    return fail(DROID_E_ARG, "ba_inputs: %s", "(E + Ei) * H * W * 2 exceeds the kernel's index range (2^62)");
  const int rows = E + Ei, mcap = nbuf < rows ? nbuf : rows;
  if (cap_e < rows) return fail(DROID_E_ARG, "ba_inputs: bad %s", "cap_e (below E + Ei)");
  if (cap_m < mcap) return fail(DROID_E_ARG, "ba_inputs: bad %s", "cap_m (below min(nbuf, E + Ei))");
  if (damping_net && n_damp < 0) return fail(DROID_E_ARG, "ba_inputs: bad %s", "n_damp (negative)");
  if (t0 < -1) return fail(DROID_E_ARG, "ba_inputs: bad %s", "t0 (>= 0, or -1 for none)");
  if (net_dtype != DROID_F16 && net_dtype != DROID_F32) return fail(DROID_E_ARG, "ba_inputs: bad %s", "net_dtype (f16 or f32)");
  if (damp_dtype != DROID_F16 && damp_dtype != DROID_F32) return fail(DROID_E_ARG, "ba_inputs: bad %s", "damp_dtype (f16 or f32)");
  if (!ii || !jj || !a || !w || !damping_buf)
    return fail(DROID_E_ARG, "ba_inputs: null %s", "pointer (ii / jj / a / w / damping_buf)");
  if (Ei > 0 && (!ii_inac || !jj_inac || !target_inac || !weight_inac))
    return fail(DROID_E_ARG, "ba_inputs: null %s", "pointer (ii_inac / jj_inac / target_inac / weight_inac) with Ei > 0");
  if (!ii_ba || !jj_ba || !target_ba || !weight_ba || !eta || !frames_active || !frames_eta || !info)
    return fail(DROID_E_ARG, "ba_inputs: null %s",
                "pointer (ii_ba / jj_ba / target_ba / weight_ba / eta / frames_active / frames_eta / info)");
  if (!delta && (target_state || weight_state))
    return fail(DROID_E_ARG, "ba_inputs: %s", "target_state / weight_state given in emit-only mode (delta is NULL)");
  if (!workspace) return fail(DROID_E_ARG, "ba_inputs: null %s", "workspace");
  const size_t ws_need = ba_inputs_workspace_bytes(E, Ei, nbuf);
  if (workspace_bytes < ws_need) return fail(DROID_E_WORKSPACE, "ba_inputs: %s", "workspace too small");
  if ((uintptr_t)workspace % 4 != 0) return fail(DROID_E_ARG, "ba_inputs: %s", "workspace is not 4-byte aligned");

  // bytes of n rows of `per` elements of `size` bytes, saturating
  auto bytes = [](uint64_t n, unsigned __int128 per, unsigned size) -> uint64_t {
    const unsigned __int128 b = n * per * size;
    return b > UINT64_MAX ? UINT64_MAX : (uint64_t)b;
  };
  const unsigned net_size = delta ? (net_dtype == DROID_F16 ? 2 : 4) : 4, damp_size = damp_dtype == DROID_F16 ? 2 : 4;
  struct Range { const void* p; uint64_t bytes; const char* name; };
  const Range ins[11] = {{ii, bytes(E, 1, 8), "ii"}, {jj, bytes(E, 1, 8), "jj"}, {a, bytes(E, hw * 2, 4), "a"},
                         {delta, delta ? bytes(E, hw * 2, net_size) : 0, "delta"}, {w, bytes(E, hw * 2, net_size), "w"},
                         {damping_net, damping_net ? bytes(n_damp, hw, damp_size) : 0, "damping_net"},
                         {ii_inac, bytes(Ei, 1, 8), "ii_inac"}, {jj_inac, bytes(Ei, 1, 8), "jj_inac"},
                         {target_inac, bytes(Ei, hw * 2, 4), "target_inac"}, {weight_inac, bytes(Ei, hw * 2, 4), "weight_inac"},
                         {nullptr, 0, ""}};
  const Range outs[12] = {{damping_buf, bytes(nbuf, hw, 4), "damping_buf"},
                          {target_state, target_state ? bytes(E, hw * 2, 4) : 0, "target_state"},
                          {weight_state, weight_state ? bytes(E, hw * 2, 4) : 0, "weight_state"},
                          {ii_ba, bytes(cap_e, 1, 8), "ii_ba"}, {jj_ba, bytes(cap_e, 1, 8), "jj_ba"},
                          {target_ba, bytes(cap_e, hw * 2, 4), "target_ba"}, {weight_ba, bytes(cap_e, hw * 2, 4), "weight_ba"},
                          {eta, bytes(cap_m, hw, 4), "eta"}, {frames_active, bytes(cap_m, 1, 8), "frames_active"},
                          {frames_eta, bytes(cap_m, 1, 8), "frames_eta"}, {info, 32, "info"}, {workspace, ws_need, "workspace"}};
  for (int o = 0; o < 12; o++) {
    const Range& out = outs[o];
    for (const Range& in : ins)
      if (bytes_overlap(out.p, out.bytes, in.p, in.bytes)) return fail(DROID_E_ARG, "ba_inputs: %s overlaps %s", out.name, in.name);
    for (int q = 0; q < o; q++)
      if (bytes_overlap(out.p, out.bytes, outs[q].p, outs[q].bytes))
        return fail(DROID_E_ARG, "ba_inputs: %s overlaps %s", out.name, outs[q].name);
  }
  BaInputsArgs x{ii, jj, a, delta, w, damping_net, damping_buf, ii_inac, jj_inac, target_inac, weight_inac, E, Ei, H, W, nbuf,
                 damping_net ? n_damp : 0, net_dtype == DROID_F16, damp_dtype == DROID_F16, t0, ep, target_state, weight_state,
                 ii_ba, jj_ba, target_ba, weight_ba, eta, frames_active, frames_eta, info, workspace};
  launch_ba_inputs(x, (hipStream_t)stream);
  return check_hip("ba_inputs");
}

// ---------------------------------------------------------------------------- corr_encode (droid_update_hip.h)
size_t droid_corr_encode_packed_bytes(void) { return DROID_CORR_ENCODE_PACKED_BYTES; }

int droid_corr_encode(const void* const* volumes, const int64_t* slots, const float* coords, const void* packed, void* out,
                      int B, int64_t cap, int H1, int W1, int radius, int levels, int out_channels, int dtype,
                      int coords_layout, void* stream) {
  if (B < 0 || B > 65535) return fail(DROID_E_ARG, "corr_encode: bad %s", "B (0 .. 65535)");
  if (H1 < 1 || W1 < 1 || (long long)H1 * W1 > (1ll << 30))
    return fail(DROID_E_ARG, "corr_encode: bad %s", "map size (H1, W1 >= 1, H1 * W1 <= 2^30)");
  if (radius != 3) return fail(DROID_E_ARG, "corr_encode: bad %s", "radius (3)");
  if (levels != 4) return fail(DROID_E_ARG, "corr_encode: bad %s", "levels (4)");
  if (out_channels != 128) return fail(DROID_E_ARG, "corr_encode: bad %s", "out_channels (128)");
  if (cap < 1 || (!slots && cap < B)) return fail(DROID_E_ARG, "corr_encode: bad %s", "cap (at least 1; at least B without slots)");
  if (coords_layout != DROID_COORDS_2HW && coords_layout != DROID_COORDS_HW2)
    return fail(DROID_E_ARG, "corr_encode: bad %s", "coords_layout (DROID_COORDS_2HW or DROID_COORDS_HW2)");
  if (dtype != DROID_F16 && dtype != DROID_F32) return fail(DROID_E_ARG, "corr_encode: bad %s", "dtype (f16 or f32)");
  if (B == 0) return DROID_OK;
  if (!volumes || !coords || !packed || !out) return fail(DROID_E_ARG, "corr_encode: null %s", "pointer");
  for (int l = 0; l < levels; l++)   // a level without pixels (H1 or W1 below 2^l) is never read and may be NULL
    if (!volumes[l] && (H1 >> l) > 0 && (W1 >> l) > 0) return fail(DROID_E_ARG, "corr_encode: null %s", "pyramid level");
  if (((uintptr_t)packed & 15) != 0) return fail(DROID_E_ARG, "corr_encode: %s", "packed is not 16-byte aligned");
  int rc = launch_corr_encode(volumes, slots, (long long)(slots ? cap : (int64_t)B), coords, packed, out, B, H1, W1, dtype,
                              coords_layout == DROID_COORDS_HW2, (hipStream_t)stream);
  if (rc) return fail(rc, "corr_encode: %s", "unsupported configuration");
  return check_hip("corr_encode");
}

// ---------------------------------------------------------------------------- motion_encode (droid_motion_encode_hip.h)
size_t droid_motion_encode_packed_bytes(void) { return DROID_CORR_ENCODE_PACKED_BYTES; }

int droid_motion_encode(const float* poses, const float* disps, const float* intrinsics, int intr_stride, const int64_t* ii,
                        const int64_t* jj, const float* target, const float* motn_in, const void* packed, float* coords,
                        float* valid, void* out, int E, int nbuf, int H, int W, int out_channels, void* stream) {
  if (E < 0 || E > 65535) return fail(DROID_E_ARG, "motion_encode: bad %s", "E (0 .. 65535)");
  if (H < 1 || W < 1 || (int64_t)H * W > ((int64_t)1 << 30))
    return fail(DROID_E_ARG, "motion_encode: bad %s", "map size (H, W >= 1, H * W <= 2^30)");
  if (nbuf < 1) return fail(DROID_E_ARG, "motion_encode: bad %s", "nbuf (at least 1)");
  if (out_channels != 128) return fail(DROID_E_ARG, "motion_encode: bad %s", "out_channels (128)");
  if (intr_stride != 0 && intr_stride != 4) return fail(DROID_E_ARG, "motion_encode: bad %s", "intr_stride (0 or 4)");
  if (E == 0) return DROID_OK;
  if (!packed || !out) return fail(DROID_E_ARG, "motion_encode: null %s", "pointer (packed, out)");
  if (((uintptr_t)packed & 15) != 0) return fail(DROID_E_ARG, "motion_encode: %s", "packed is not 16-byte aligned");
  if (!motn_in && (!poses || !disps || !intrinsics || !ii || !jj || !target || !coords || !valid))
    return fail(DROID_E_ARG, "motion_encode: null %s", "pointer (the geometry source and coords, valid, or motn_in)");
  launch_motion_encode(poses, disps, intrinsics, intr_stride, ii, jj, target, motn_in, packed, coords, valid, out, E, nbuf, H,
                       W, (hipStream_t)stream);
  return check_hip("motion_encode");
}

// ---------------------------------------------------------------------------- update_heads (droid_heads_hip.h)
size_t droid_head_packed_bytes(int n_out) {
  if (n_out != 1 && n_out != 2) return 0;
  return (((size_t)(1152 + 1) * n_out * sizeof(float)) + 15) / 16 * 16;
}

int droid_update_heads(const void* const* x, const void* const* packed, void* const* out, const int* n_out, const int* act,
                       int heads, int B, int H, int W, int in_channels, void* stream) {
  if (heads != 1 && heads != 2) return fail(DROID_E_ARG, "update_heads: bad %s", "heads (1 or 2)");
  if (B < 0 || B > 65535) return fail(DROID_E_ARG, "update_heads: bad %s", "B (0 .. 65535)");
  if (H < 1 || W < 1 || (int64_t)H * W > ((int64_t)1 << 30))
    return fail(DROID_E_ARG, "update_heads: bad %s", "map size (H, W >= 1, H * W <= 2^30)");
  if (in_channels != 128) return fail(DROID_E_ARG, "update_heads: bad %s", "in_channels (128)");
  for (int k = 0; n_out && k < heads; k++)
    if (n_out[k] != 1 && n_out[k] != 2) return fail(DROID_E_ARG, "update_heads: bad %s", "n_out (1 or 2)");
  for (int k = 0; act && k < heads; k++)
    if (act[k] < DROID_HEAD_IDENTITY || act[k] > DROID_HEAD_SOFTPLUS_CENTI)
      return fail(DROID_E_ARG, "update_heads: bad %s", "act (DROID_HEAD_IDENTITY, _SIGMOID or _SOFTPLUS_CENTI)");
  if (B == 0) return DROID_OK;
  if (!x || !packed || !out || !n_out || !act)
    return fail(DROID_E_ARG, "update_heads: null %s", "pointer (x, packed, out, n_out, act)");
  for (int k = 0; k < heads; k++)
    if (!x[k] || !packed[k] || !out[k]) return fail(DROID_E_ARG, "update_heads: null %s", "pointer (an entry of x, packed, out)");
  for (int k = 0; k < heads; k++)
    if (((uintptr_t)packed[k] & 15) != 0) return fail(DROID_E_ARG, "update_heads: %s", "packed is not 16-byte aligned");
  launch_update_heads(x, packed, out, n_out, act, heads, B, H, W, (hipStream_t)stream);
  return check_hip("update_heads");
}

// ---------------------------------------------------------------------------- conv3x3 (droid_conv3x3_hip.h)
static bool conv3x3_sizes(int c_in, int c_out) {
  return c_in >= 32 && c_in <= 512 && c_in % 32 == 0 && c_out >= 64 && c_out <= 256 && c_out % 64 == 0;
}

size_t droid_conv3x3_packed_bytes(int c_in, int c_out) {
  if (!conv3x3_sizes(c_in, c_out)) return 0;
  return ((size_t)9 * c_in * c_out + c_out) * 2;
}

int droid_conv3x3(const void* x, const void* packed, void* y, int B, int c_in, int c_out, int H, int W,
                  int64_t x_batch_stride, int64_t y_batch_stride, int64_t y_group_stride, int group_channels, int relu,
                  void* stream) {
  if (B < 0 || B > 65535) return fail(DROID_E_ARG, "conv3x3: bad %s", "B (0 .. 65535)");
  if (c_in < 32 || c_in > 512 || c_in % 32 != 0) return fail(DROID_E_ARG, "conv3x3: bad %s", "c_in (a multiple of 32 in 32 .. 512)");
  if (c_out < 64 || c_out > 256 || c_out % 64 != 0)
    return fail(DROID_E_ARG, "conv3x3: bad %s", "c_out (a multiple of 64 in 64 .. 256)");
  if (H < 1 || W < 1 || (int64_t)H * W > ((int64_t)1 << 30))
    return fail(DROID_E_ARG, "conv3x3: bad %s", "map size (H, W >= 1, H * W <= 2^30)");
  if (group_channels < 64 || group_channels % 64 != 0 || c_out % group_channels != 0)
    return fail(DROID_E_ARG, "conv3x3: bad %s", "group_channels (a multiple of 64 that divides c_out)");
  if (relu != 0 && relu != 1) return fail(DROID_E_ARG, "conv3x3: bad %s", "relu (0 or 1)");
  const int64_t HW = (int64_t)H * W;
  if (B > 1 && x_batch_stride < c_in * HW) return fail(DROID_E_ARG, "conv3x3: bad %s", "x_batch_stride (below c_in * H * W)");
  if (B > 1 && y_batch_stride < group_channels * HW)
    return fail(DROID_E_ARG, "conv3x3: bad %s", "y_batch_stride (below group_channels * H * W)");
  if (B == 0) return DROID_OK;
  if (!x || !packed || !y) return fail(DROID_E_ARG, "conv3x3: null %s", "pointer (x, packed, y)");
  if (((uintptr_t)packed & 15) != 0) return fail(DROID_E_ARG, "conv3x3: %s", "packed is not 16-byte aligned");
  launch_conv3x3(x, packed, y, B, c_in, c_out, H, W, x_batch_stride, y_batch_stride, y_group_stride, group_channels, relu,
                 (hipStream_t)stream);
  return check_hip("conv3x3");
}

// ---------------------------------------------------------------------------- conv_gru (droid_gru_hip.h)
static bool gru_c_in_ok(int c_in) { return c_in >= 160 && c_in <= 512 && c_in % 32 == 0; }
static bool gru_map_ok(int H, int W) { return H >= 1 && W >= 1 && (int64_t)H * W <= ((int64_t)1 << 30); }

size_t droid_gru_packed_bytes(int c_in) { return gru_c_in_ok(c_in) ? gru_packed_bytes(c_in) : 0; }

size_t droid_gru_workspace_bytes(int B, int H, int W) {
  if (B < 0 || B > 65535 || !gru_map_ok(H, W)) return 0;
  return gru_workspace_bytes(B, H, W);
}

// the size checks every segment call shares, in the header's order; *c_in_out = the channel sum
static int gru_check_sizes(const void* const* seg, const int64_t* seg_batch_stride, const int* seg_channels, int nseg, int B,
                           int H, int W, int* c_in_out) {
  if (B < 0 || B > 65535) return fail(DROID_E_ARG, "conv_gru: bad %s", "B (0 .. 65535)");
  if (nseg < 2 || nseg > 5) return fail(DROID_E_ARG, "conv_gru: bad %s", "nseg (2 .. 5)");
  if (!seg || !seg_batch_stride || !seg_channels)
    return fail(DROID_E_ARG, "conv_gru: null %s", "array (seg, seg_batch_stride, seg_channels)");
  int c_in = 0;
  for (int k = 0; k < nseg; k++) {
    if (seg_channels[k] < 32 || seg_channels[k] > 512 || seg_channels[k] % 32 != 0 || (k == 0 && seg_channels[k] != 128))
      return fail(DROID_E_ARG, "conv_gru: bad seg_channels[%d] (a positive multiple of 32; seg_channels[0] is 128)", k);
    c_in += seg_channels[k];
  }
  if (!gru_c_in_ok(c_in)) return fail(DROID_E_ARG, "conv_gru: bad %s", "c_in (the channel sum, a multiple of 32 in 160 .. 512)");
  if (!gru_map_ok(H, W)) return fail(DROID_E_ARG, "conv_gru: bad %s", "map size (H, W >= 1, H * W <= 2^30)");
  const int64_t HW = (int64_t)H * W;
  for (int k = 0; k < nseg; k++)
    if (B > 1 && seg_batch_stride[k] < seg_channels[k] * HW)
      return fail(DROID_E_ARG, "conv_gru: bad seg_batch_stride[%d] (below seg_channels * H * W)", k);
  *c_in_out = c_in;
  return DROID_OK;
}

static bool gru_null_segment(const void* const* seg, int nseg) {
  for (int k = 0; k < nseg; k++)
    if (!seg[k]) return true;
  return false;
}

int droid_gru_context(const void* net, int64_t net_batch_stride, const void* packed, int c_in, int B, int H, int W, float* g,
                      void* ws, size_t ws_bytes, void* stream) {
  if (B < 0 || B > 65535) return fail(DROID_E_ARG, "conv_gru: bad %s", "B (0 .. 65535)");
  if (!gru_c_in_ok(c_in)) return fail(DROID_E_ARG, "conv_gru: bad %s", "c_in (the channel sum, a multiple of 32 in 160 .. 512)");
  if (!gru_map_ok(H, W)) return fail(DROID_E_ARG, "conv_gru: bad %s", "map size (H, W >= 1, H * W <= 2^30)");
  if (B > 1 && net_batch_stride < 128 * (int64_t)H * W)
    return fail(DROID_E_ARG, "conv_gru: bad %s", "net_batch_stride (below 128 * H * W)");
  if (ws_bytes < gru_context_workspace_bytes(B, H, W))
    return fail(DROID_E_ARG, "conv_gru: %s", "ws_bytes is below B * ceil(H * W / 256) * 512");
  if (B == 0) return DROID_OK;
  if (!net || !packed || !g || !ws) return fail(DROID_E_ARG, "conv_gru: null %s", "pointer (net, packed, g, ws)");
  if ((((uintptr_t)packed | (uintptr_t)ws) & 15) != 0) return fail(DROID_E_ARG, "conv_gru: %s", "packed or ws is not 16-byte aligned");
  launch_gru_context(net, net_batch_stride, packed, c_in, B, H, W, g, ws, (hipStream_t)stream);
  return check_hip("conv_gru");
}

int droid_gru_gates(const void* const* seg, const int64_t* seg_batch_stride, const int* seg_channels, int nseg,
                    const void* packed, const float* g, void* z, void* rnet, int B, int H, int W, void* stream) {
  int c_in = 0;
  if (int rc = gru_check_sizes(seg, seg_batch_stride, seg_channels, nseg, B, H, W, &c_in)) return rc;
  if (B == 0) return DROID_OK;
  if (gru_null_segment(seg, nseg) || !packed || !g || !z || !rnet)
    return fail(DROID_E_ARG, "conv_gru: null %s", "pointer (seg[k], packed, g, z, rnet)");
  if (((uintptr_t)packed & 15) != 0) return fail(DROID_E_ARG, "conv_gru: %s", "packed is not 16-byte aligned");
  launch_gru_gates(seg, seg_batch_stride, seg_channels, nseg, packed, g, z, rnet, B, H, W, (hipStream_t)stream);
  return check_hip("conv_gru");
}

int droid_gru_update(const void* const* seg, const int64_t* seg_batch_stride, const int* seg_channels, int nseg,
                     const void* packed, const float* g, const void* z, const void* net, int64_t net_batch_stride,
                     void* out, int64_t out_batch_stride, int B, int H, int W, void* stream) {
  int c_in = 0;
  if (int rc = gru_check_sizes(seg, seg_batch_stride, seg_channels, nseg, B, H, W, &c_in)) return rc;
  if (B > 1 && net_batch_stride < 128 * (int64_t)H * W)
    return fail(DROID_E_ARG, "conv_gru: bad %s", "net_batch_stride (below 128 * H * W)");
  if (B > 1 && out_batch_stride < 128 * (int64_t)H * W)
    return fail(DROID_E_ARG, "conv_gru: bad %s", "out_batch_stride (below 128 * H * W)");
  if (B == 0) return DROID_OK;
  if (gru_null_segment(seg, nseg) || !packed || !g || !z || !net || !out)
    return fail(DROID_E_ARG, "conv_gru: null %s", "pointer (seg[k], packed, g, z, net, out)");
  if (((uintptr_t)packed & 15) != 0) return fail(DROID_E_ARG, "conv_gru: %s", "packed is not 16-byte aligned");
  launch_gru_update(seg, seg_batch_stride, seg_channels, nseg, packed, g, z, net, net_batch_stride, out, out_batch_stride, B, H,
                    W, (hipStream_t)stream);
  return check_hip("conv_gru");
}

int droid_conv_gru(const void* const* seg, const int64_t* seg_batch_stride, const int* seg_channels, int nseg,
                   const void* packed, void* out, int64_t out_batch_stride, int B, int H, int W, void* ws, size_t ws_bytes,
                   void* stream) {
  int c_in = 0;
  if (int rc = gru_check_sizes(seg, seg_batch_stride, seg_channels, nseg, B, H, W, &c_in)) return rc;
  if (B > 1 && out_batch_stride < 128 * (int64_t)H * W)
    return fail(DROID_E_ARG, "conv_gru: bad %s", "out_batch_stride (below 128 * H * W)");
  if (ws_bytes < gru_workspace_bytes(B, H, W)) return fail(DROID_E_ARG, "conv_gru: %s", "ws_bytes is below droid_gru_workspace_bytes");
  if (B == 0) return DROID_OK;
  if (gru_null_segment(seg, nseg) || !packed || !out || !ws)
    return fail(DROID_E_ARG, "conv_gru: null %s", "pointer (seg[k], packed, out, ws)");
  if ((((uintptr_t)packed | (uintptr_t)ws) & 15) != 0) return fail(DROID_E_ARG, "conv_gru: %s", "packed or ws is not 16-byte aligned");
  // ws: the context partials, g [B,3,128] fp32, z, rnet [B,128,H,W] half
  char* base = static_cast<char*>(ws);
  float* g = reinterpret_cast<float*>(base + gru_context_workspace_bytes(B, H, W));
  char* z = reinterpret_cast<char*>(g) + (size_t)B * 3 * 128 * sizeof(float);
  const size_t plane = (gru_workspace_bytes(B, H, W) - (size_t)(z - base)) / 2;
  char* rnet = z + plane;
  hipStream_t s = (hipStream_t)stream;
  launch_gru_context(seg[0], seg_batch_stride[0], packed, c_in, B, H, W, g, ws, s);
  launch_gru_gates(seg, seg_batch_stride, seg_channels, nseg, packed, g, z, rnet, B, H, W, s);
  const void* seg_q[5];
  int64_t stride_q[5];
  for (int k = 0; k < nseg; k++) {
    seg_q[k] = seg[k];
    stride_q[k] = seg_batch_stride[k];
  }
  seg_q[0] = rnet;
  stride_q[0] = 128 * (int64_t)H * W;
  launch_gru_update(seg_q, stride_q, seg_channels, nseg, packed, g, z, seg[0], seg_batch_stride[0], out, out_batch_stride, B, H,
                    W, s);
  return check_hip("conv_gru");
}

}  // extern "C"
