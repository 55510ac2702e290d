/*
 * droid_update_hip.h -- C ABI of the update-loop operators that sit between the update network and `ba`.  A second
 * header next to droid_backends_hip.h with the same conventions: raw DEVICE pointers, sizes and a HIP stream (void*, a
 * hipStream_t); 0 on success, a negative DROID_E_* code on a contract violation the host can see, with a thread-local
 * message (droid_last_error); every function enqueues on `stream` and returns without synchronising.  The library
 * (libdroid_backends_hip.so) and DROID_ABI_VERSION are the main header's.
 */
#ifndef DROID_UPDATE_HIP_H
#define DROID_UPDATE_HIP_H

#include "droid_backends_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tail of `FactorGraph.update` from the update operator's outputs to the arguments of `ba`
 * (droid_slam/factor_graph.py:213-238, and the per-step tail of update_lowmem, :292-294):
 *   t0 = max(1, ii.min() + 1) ; target = coords1 + delta.float() ; weight = weight.float()
 *   damping_buf[unique(ii)] = damping ; m = (ii_inac >= t0 - 3) & (jj_inac >= t0 - 3)
 *   ii, jj, target, weight = cat(x_inac[m], x) ; eta = .2 * damping_buf[unique(ii)] + EP
 *   target, weight -> view(-1, h, w, 2).permute(0, 3, 1, 2).contiguous() ; t1 = max(ii.max(), jj.max()) + 1
 * in two launches on the stream -- a one-workgroup prepare launch and a streaming launch -- without atomics; the host
 * never reads an index, and a caller reads at most the 8 ints of `info`.  Not one of the reference's nine operators.
 *
 * Inputs.  All on one device, contiguous, only read unless stated otherwise.
 *   ii, jj [E] int64: the active edges, E >= 1.
 *   a [E,H,W,2] f32: `coords1` in absorb mode, the held `target` in emit-only mode.
 *   delta [E,H,W,2] of net_dtype (DROID_F16 or DROID_F32), or NULL.  NULL is emit-only mode: nothing is added to a.
 *   w [E,H,W,2]: net_dtype in absorb mode, f32 in emit-only mode.
 *   damping_net [n_damp,H,W] of damp_dtype (DROID_F16 or DROID_F32), or NULL (then n_damp is not looked at).
 *   damping_buf [nbuf,H,W] f32, read and written.
 *   ii_inac, jj_inac [Ei] int64 ; target_inac, weight_inac [Ei,H,W,2] f32.  Ei >= 0; these are NULL when Ei = 0.
 *   t0: >= 0, or -1 for the reference's `None`.   ep: float.
 *
 * Prepare launch.  Every index value is compared as the int64 it is.
 *  1. t0' = t0 if t0 >= 0, else max(1, min_e ii[e] + 1).
 *  2. Inactive edge k is kept iff ii_inac[k] >= t0' - 3 && jj_inac[k] >= t0' - 3.  K is the number kept.
 *  3. The emitted edge list is the kept inactive edges in their order, then the E active edges in their order;
 *     Eb = K + E.  ii_ba, jj_ba [cap_e] int64 receive the list.
 *  4. A is the set of distinct in-range values of the active ii, ascending, |A| = G; U the set of distinct in-range
 *     values of the emitted ii, ascending, |U| = M.  In range means inside [0, nbuf).  frames_active [cap_m] int64
 *     receives A (torch.unique(self.ii): what the upsampling takes as ix), frames_eta [cap_m] int64 receives U.
 *  5. info, 8 device ints: {Eb, M, G, t0', 1 + max over the emitted ii and jj, flags, K, 0}; t0' and the maximum are
 *     saturated to the range of int.
 *     flags bit 0: an emitted ii or jj lies outside [0, nbuf).  The edge is emitted as it is, so that `ba` reports it in
 *       its own status word; it creates no row of A or U and touches no damping row.
 *     flags bit 1: damping_net is given and n_damp != G.
 *
 * Streaming launch.  All arithmetic is fp32; halves are widened exactly; nothing is sanitised.
 *   Active edge e: t = a[e] + float(delta[e]), one IEEE addition (emit-only mode: t = a[e]); wt = float(w[e]).
 *   With the state outputs given (absorb mode only): target_state[e] = t, weight_state[e] = wt, as [E,H,W,2].
 *   BA row r of the emitted list: target_ba[r, c, y, x] and weight_ba[r, c, y, x], c = 0, 1, hold component c of the
 *     edge's target and weight at pixel (y, x) -- view(-1, h, w, 2).permute(0, 3, 1, 2).contiguous().  A kept inactive
 *     edge copies target_inac[k] and weight_inac[k].
 *   Frame f = A[g] with g < n_damp: damping_buf[f] = float(damping_net[g]).  No other row of damping_buf is written.
 *   Row i with f = U[i]: d is the value just written if f is in A and its row was written, else the stored
 *     damping_buf[f]; eta[i] = fl(fl(0.2f * d) + ep): two roundings, never a fused multiply-add.
 *   Rows at and beyond Eb of the edge outputs are NOT written; rows at and beyond M of eta and frames_eta, and at and
 *   beyond G of frames_active, are NOT written.  A given edge's bits do not depend on E, Ei or its row.  The same bits
 *   on every run, with any workspace contents.  No alignment requirement: where a row's start is not 16-byte aligned
 *   (every other row when H * W is odd) or H * W is no multiple of 4, an element-wise path computes the same bits as the
 *   16-byte path.
 *
 * Refusals, DROID_E_ARG with a message that names ba_inputs and the argument, before any HIP call, sizes before
 * pointers: E < 1 ; Ei < 0 ; E + Ei > 65535 ; nbuf < 1 or above DROID_BA_INPUTS_MAX_NBUF (the prepare launch keeps two
 * presence maps, their bitmaps and prefix ranks in LDS) ; H or W < 1, or (E + Ei) * H * W * 2 beyond 2^62 ;
 * cap_e < E + Ei ; cap_m < min(nbuf, E + Ei) ; n_damp < 0 with damping_net given ; t0 < -1 ; a dtype code other than
 * F16 / F32 ; a null required pointer ; inactive pointers null while Ei > 0 ; state outputs given while delta is NULL ;
 * any output, the workspace included, sharing a byte with an input or with another output (damping_buf is the one
 * in/out argument and may share a byte with nothing else).
 * Workspace: droid_ba_inputs_workspace_bytes(E, Ei, nbuf) is host arithmetic (4 + E + Ei + 2 min(nbuf, E + Ei) ints)
 * and returns 0 for sizes refused here; 4-byte aligned; a workspace that is too small gives DROID_E_WORKSPACE.
 * Concurrent calls need separate workspaces. */
#define DROID_BA_INPUTS_MAX_NBUF 16384
size_t droid_ba_inputs_workspace_bytes(int E, int Ei, int nbuf);
int droid_ba_inputs(const int64_t *ii, const int64_t *jj, const float *a, const void *delta, const void *w,
                    const void *damping_net, float *damping_buf, const int64_t *ii_inac, const int64_t *jj_inac,
                    const float *target_inac, const float *weight_inac, int E, int Ei, int H, int W, int nbuf,
                    int n_damp, int net_dtype, int damp_dtype, int t0, float ep, float *target_state,
                    float *weight_state, int64_t *ii_ba, int64_t *jj_ba, float *target_ba, float *weight_ba, int cap_e,
                    float *eta, int64_t *frames_active, int64_t *frames_eta, int cap_m, int *info, void *workspace,
                    size_t workspace_bytes, void *stream);

/* The correlation lookup of an update step fused with the first two layers of the update module's correlation encoder:
 * `CorrBlock.__call__` (droid_slam/modules/corr.py:40-50) followed by `corr_encoder[0:2]`, a Conv2d(196, 128, 1) and a
 * ReLU under autocast (droid_slam/droid_net.py:83-87, :125), in ONE launch that never writes the [B,196,H1,W1] lookup:
 *
 *   y[e, n, p] = relu( half( sum_k a[e,k,p] * w16[n,k]  +  float(b16[n]) ) )          y: [B, 128, H1, W1] half
 *
 * a[e,k,p], k = l * 49 + (ix * 7 + iy), is the value droid_corr_pyramid_forward[_slots] yields for channel k of entry e
 *   at pixel p -- the channel order of torch.cat(out_pyramid).  Half pyramids: those bits.  fp32 pyramids: that fp32
 *   value rounded to half, nearest-even, overflow to inf (autocast's cast in front of the convolution).  Everything the
 *   lookup does is inherited, because the kernel calls the lookup's own device functions: border masking, empty windows,
 *   zeros for non-finite coordinates, the exact 2^-l scaling of the coordinates.
 * w16 = half(weight), b16 = half(bias), nearest-even from the fp32 parameters (autocast's cast).
 * Arithmetic: every product a * w16 is exact in fp32; fp32 accumulation (v_mfma_f32_16x16x32_f16), in an order that is
 *   fixed but not specified; then + float(b16[n]) in fp32, ONE rounding to half, then max(., 0) (+0 for every value not
 *   above zero; a NaN stays a NaN).  No atomics: the same bits on every run, and the bits of an entry do not depend on
 *   B, on its position in the batch or on its slot.
 * slots: NULL, or [B] int64 on the DEVICE as in droid_corr_pyramid_forward_slots: the levels are capacity buffers
 *   [cap,H1,W1,H1>>l,W1>>l] and entry e reads slot slots[e].  A slot outside [0, cap) gives a = 0 for that entry, so
 *   its output is relu(b16[n]) everywhere; nothing outside the buffers is read; two entries may name one slot.  With
 *   slots NULL entry e reads entry e of [cap,...] buffers, cap >= B.
 * coords: fp32, DROID_COORDS_2HW = [B,2,H1,W1] (x plane, y plane: what the lookup takes) or DROID_COORDS_HW2 =
 *   [B,H1,W1,2] (`coords1[0]` as reproject / motion_features return it).  The values used are the same either way.
 * Shapes: radius 3, 4 levels, 128 output channels (the reference's cor_planes), any H1, W1 >= 1 (a level with
 *   H1 >> l == 0 or W1 >> l == 0 has no taps, contributes zeros, and its pointer is not looked at), B <= 65535.
 *
 * packed: the parameters, packed once per network.  DROID_CORR_ENCODE_PACKED_BYTES bytes, 16-byte aligned:
 *   halves [4 levels][2 K steps][8 channel tiles][64 lanes][8], then b16 [128].  K is padded per level from 49 to 64:
 *   element (l, s, nt, lane, j) is w16[n][l * 49 + kk] with n = 16 nt + (lane & 15), kk = 32 s + 8 (lane >> 4) + j, and
 *   ZERO where kk >= 49.  Lane `lane` of a wave thus fetches its B fragment of v_mfma_f32_16x16x32_f16 for (level l,
 *   K step s, channel tile nt) with one 16-byte load, and a wave's 64 loads are one contiguous KiB.  The kernel writes
 *   the padding columns 49..63 of its own LDS A tile as zeros itself, whatever the LDS held before.
 *
 * Refusals, DROID_E_ARG with a message that names corr_encode and the argument, before any HIP call, sizes before
 * dtypes before pointers: B outside [0, 65535] ; H1 or W1 < 1 or H1 * W1 > 2^30 ; radius != 3 ; levels != 4 ;
 * out_channels != 128 ; cap < 1, or cap < B without slots ; a coords_layout that is neither constant ; a dtype other
 * than F16 / F32 (F64 is refused) ; then, for B > 0: a null volumes / coords / packed / out, a null level that has
 * pixels, a packed buffer that is not 16-byte aligned.  B == 0 launches nothing and returns DROID_OK.  There is no
 * fallback: the unfused sequence stays available.
 * The two prototypes, droid_corr_encode_packed_bytes (host arithmetic: the constant below) and droid_corr_encode, are in
 * droid_corr_encode_hip.h, included at the end of this header: tests/test_ba_inputs_abi.py pins the prototypes written
 * in this file, like tests/test_abi.py those of the main header. */
#define DROID_COORDS_2HW 0
#define DROID_COORDS_HW2 1
#define DROID_CORR_ENCODE_PACKED_BYTES (4 * 64 * 128 * 2 + 128 * 2)

#ifdef __cplusplus
}
#endif
#include "droid_corr_encode_hip.h"
#endif /* DROID_UPDATE_HIP_H */
