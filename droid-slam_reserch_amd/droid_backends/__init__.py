"""droid_backends -- MI355X (gfx950) drop-in for the reference's `droid_backends` extension.

Same nine operators, argument order and return structure as the pybind module of
/root/reference/src/droid.cpp:237-250, so `droid_slam/depth_video.py`, `factor_graph.py` and
`modules/corr.py` import and call it unchanged on PyTorch-ROCm.  This file is the host-side
mirror of droid.cpp: contiguity checks + thin calls into the C ABI
(include/droid_backends_hip.h, libdroid_backends_hip.so) on PyTorch's current HIP stream.
PyTorch is plumbing only (device memory, streams); all arithmetic is in the HIP library.
"""
from __future__ import annotations

import ctypes
import os as _os

import torch

from . import _lib
from ._args import ScratchCache, _ptr, _stream, _ws_key, check_tensors
from ._lib import DroidBackendError  # noqa: F401
from .ba_binding import BAProblemDev, BaBinding, read_status
from . import se3
from .se3 import SE3
from .se3 import interpolate as pose_interpolate
from .update_tail import BaInputs, ba_inputs
from .corr_encode import CorrEncoder
from .motion_encode import FlowEncoder
from .update_heads import UpdateHeads
from .conv3x3 import Conv3x3
from .conv_gru import ConvGRU

__all__ = ["ba", "frame_distance", "projmap", "depth_filter", "iproj", "altcorr_forward",
           "altcorr_backward", "corr_index_forward", "corr_index_backward",
           "altcorr_pyramid_forward", "reproject", "motion_features", "frame_distance_matrix",
           "corr_pyramid_forward",  # the last four are additions
           "proximity_edges",       # add_proximity_factors' edge selection, on the device
           "corr_volume_pyramid",   # CorrBlock.__init__ for a list of edges, in one launch
           "upsample_disps", "cvx_upsample",   # DepthVideo.upsample / droid_net.cvx_upsample, in one launch
           "graph_mean", "scatter_mean",       # GraphAgg's source-frame mean (torch_scatter.scatter_mean), no atomics
           "SE3", "pose_interpolate",          # the pose algebra of the inference path without lietorch (droid_backends.se3)
           "point_cloud", "PointCloud",        # the viewers' filtered, coloured map of dirty keyframes, compacted on the device
           "ba_inputs", "BaInputs",            # FactorGraph.update's tail from the network's outputs to the arguments of ba
           "CorrEncoder",                      # the lookup fused with corr_encoder[0:2] (droid_backends.corr_encode)
           "FlowEncoder",                      # reproject + motion features fused with flow_encoder[0:2] (droid_backends.motion_encode)
           "UpdateHeads",                      # the last layers of delta, weight and eta in one launch each (droid_backends.update_heads)
           "Conv3x3",                          # the 3 x 3 convolutions + ReLU in between, on the f16 matrix cores (droid_backends.conv3x3)
           "ConvGRU"]                          # the ConvGRU in four launches, its inputs read where they lie (droid_backends.conv_gru)
# droid_backends.pyramid_store (SlotTable, PyramidStore): the capacity buffers behind `self.corr` of a factor graph

_DT = {torch.float16: _lib.DROID_F16, torch.float32: _lib.DROID_F32, torch.float64: _lib.DROID_F64}
_workspaces = {}   # (device index, stream handle) -> BaBinding: grow-only scratch of that stream's `ba` calls + status mirror

# Contract violations only a kernel can see (edge index outside the buffer, eta rows != depth slots, a stalled
# solver grid) are written to a status word.  DROID_HIP_CHECK=1: read it back after every call (one sync) and
# raise.  Default: no sync -- the last kernel of a call also writes the word to page-locked host memory, and the
# NEXT `ba` call on the same (device, stream) raises if the previous one had reported a violation by then.
_SYNC_CHECK = _os.environ.get("DROID_HIP_CHECK", "0") == "1"


F32, I64, F16_OR_F32 = torch.float32, torch.int64, (torch.float16, torch.float32)


def _state(poses, disps, intrinsics):
    """The three float32 tensors most operators start with, as `check_tensors` takes them."""
    return [(poses, "poses", F32), (disps, "disps", F32), (intrinsics, "intrinsics", F32)]


def _workspace_obj(device):
    key = _ws_key(device)
    return _workspaces.get(key) or _workspaces.setdefault(key, BaBinding())


def ba_status(workspace=None):
    """(status, depth_slots) of the last `ba` on the current device and stream (blocking read)."""
    if workspace is not None:
        return read_status(_lib.load(), workspace)
    obj = _workspaces.get(_ws_key(torch.device("cuda")))
    if obj is None or obj.buf is None:
        return 0, 0
    st = obj.status()
    obj.seen = int(obj.mirror[2])   # droid_ba_status synchronised: the caller has seen everything up to here
    return st


_STATUS_TEXT = {1: "edge index outside the pose buffer", 2: "eta rows != number of depth slots "
                "|unique(ii) U [t0,t1)|", 4: "Cholesky failed (dx = 0)",
                8: "the single-launch solver stalled: another spinning grid held the GPU (dx = 0); "
                   "set DROID_CHOL_COOPERATIVE=1 or DROID_CHOL_MULTI_LAUNCH=1 when several processes share the GPU"}


def _raise_on_status(st, m, when=""):
    # bit 4 (not positive definite => dx = 0) is the reference's silent behaviour (droid_kernels.cu:1207-1210)
    bad = [txt for bit, txt in _STATUS_TEXT.items() if (st & bit) and bit != 4]
    if bad:
        raise RuntimeError(f"droid_backends.ba{when}: " + "; ".join(bad) + f" (device counted {m} depth slots)")


def ba(poses, disps, intrinsics, disps_sens, targets, weights, eta, ii, jj, t0, t1, iterations,
       lm, ep, motion_only):
    """Dense bundle adjustment, droid.cpp:88-117 -> ba_cuda droid_kernels.cu:1314-1434.

    poses [nbuf,7] and disps [nbuf,H,W] are updated in place; returns [dx, dz] like the
    reference (dz is an empty tensor when motion_only, where the reference returns an undefined
    one).  eta is not contiguity-checked, as in the reference (droid.cpp:105-112), but it is
    made contiguous here because the kernels index it directly.
    """
    _lib.load()
    check_tensors("ba", [(targets, "targets", F32), (weights, "weights", F32), (poses, "poses", F32), (disps, "disps", F32),
                         (intrinsics, "intrinsics", F32), (disps_sens, "disps_sens", F32), (ii, "ii", I64), (jj, "jj", I64)])
    motion_only = bool(motion_only)
    H, W = disps.shape[1:]
    dev = poses.device
    eta_c = None if motion_only else eta.contiguous().to(torch.float32).view(-1, H * W)
    p = BAProblemDev(poses, disps, intrinsics, disps_sens, targets, weights, eta_c, ii, jj)
    wso = _workspace_obj(dev)
    # Deferred error report, no sync: the device counts the iterations that ended with a violation or a stalled solve
    # in page-locked host memory and ORs their bits (sticky: a later call cannot overwrite them); raise once per count.
    nerr = int(wso.mirror[2])
    if nerr != wso.seen:
        wso.seen = nerr
        _raise_on_status(int(wso.mirror[3]) & ~4, int(wso.mirror[1]), " (an earlier call on this stream)")
    E, nbuf, H, W, M, t0, t1 = wso.begin(p, t0, t1, motion_only, dev)
    dx = torch.empty((max(t1 - t0, 0), 6), dtype=torch.float32, device=dev)
    dz = torch.empty((M, H * W), dtype=torch.float32, device=dev)
    wso.ba(p, iterations, lm, ep, motion_only, dx, dz)
    if _SYNC_CHECK:
        st = wso.status()
        wso.seen = int(wso.mirror[2])
        _raise_on_status(*st)
    return [dx, dz]


def frame_distance(poses, disps, intrinsics, ii, jj, beta):
    """droid.cpp:120-136 -> frame_distance_cuda droid_kernels.cu:1438-1460."""
    lib = _lib.load()
    check_tensors("frame_distance", _state(poses, disps, intrinsics) + [(ii, "ii", I64), (jj, "jj", I64)])
    nbuf, H, W = disps.shape
    nbuf = min(int(nbuf), int(poses.shape[0]))
    E = int(ii.shape[0])
    dist = torch.zeros((E,), dtype=torch.float32, device=poses.device)
    _lib.check(lib.droid_frame_distance(poses.data_ptr(), disps.data_ptr(), intrinsics.data_ptr(),
                                        ii.data_ptr(), jj.data_ptr(), E, nbuf, H, W, float(beta),
                                        dist.data_ptr(), _stream()), "frame_distance")
    return dist


def frame_distance_matrix(poses, disps, intrinsics, n, beta, bidirectional=True):
    """`DepthVideo.distance(ii=None)` (droid_slam/depth_video.py:160-190) in one launch: the [n, n] matrix of frame
    distances between the first n frames, d[i, j] = .5 * (frame_distance(i -> j) + frame_distance(j -> i)) when
    `bidirectional` (the reference's default), else frame_distance(i -> j).  No meshgrid index tensors, one kernel
    instead of two, each depth map fetched once per 32 targets.  An addition."""
    lib = _lib.load()
    check_tensors("frame_distance_matrix", _state(poses, disps, intrinsics))
    nbuf, H, W = disps.shape
    nbuf = min(int(nbuf), int(poses.shape[0]))
    n = int(n)
    d = torch.empty((n, n), dtype=torch.float32, device=poses.device)
    _lib.check(lib.droid_frame_distance_matrix(poses.data_ptr(), disps.data_ptr(), intrinsics.data_ptr(), n, nbuf,
                                               int(H), int(W), float(beta), d.data_ptr(), _stream()),
               "frame_distance_matrix")
    return .5 * (d + d.t()) if bidirectional else d


_prox_ws = ScratchCache()   # _ws_key(device) -> grow-only uint8 scratch of proximity_edges


def _forced_before(i, m):
    """sum over k < i of min(k, m): edges (i, j) step 4 emits for the frames before frame i."""
    return i * (i - 1) // 2 if i <= m + 1 else m * (m + 1) // 2 + (i - 1 - m) * m


def proximity_edge_bound(t, t0, t1, rad, max_factors, stereo):
    """Most edges one selection can return (include/droid_backends_hip.h, droid_proximity_edges: `cap`)."""
    if t <= t0:
        return 0
    forced = (t - t0 if stereo else 0) + 2 * (_forced_before(t, rad + 1) - _forced_before(t0, rad + 1))
    return max(forced, min(max_factors + 2, forced + 2 * (t - t0) * (t - t1)))


def proximity_edges(poses, disps, intrinsics, t, t0, t1, rad, nms, beta, thresh, max_factors, stereo,
                    sup_ii, sup_jj, known_ii=None, known_jj=None, dist=None):
    """The edges `FactorGraph.add_proximity_factors(t0, t1, rad, nms, beta, thresh)` adds
    (droid_slam/factor_graph.py:315-379), selected on the device: returns (ii, jj), int64, in the reference's order.

    t = frames in use (`video.counter.value`), max_factors / stereo = `graph.max_factors` / `video.stereo`;
    sup_ii / sup_jj = the edges that suppress their neighbourhood (cat of active, bad and inactive edges);
    known_ii / known_jj (optional) = active + inactive edges: with them the result is already what
    `__filter_repeated_edges` (:44-55) would leave.  The frame-distance matrix is computed here with one
    droid_frame_distance_matrix launch unless `dist` -- a DIRECTED [n, n] float32 matrix, n >= t, as that operator
    writes it -- is given (then poses / disps / intrinsics are not looked at).  The contract, with the points where
    it settles what the reference leaves open, is in include/droid_backends_hip.h.  One synchronisation: the edge
    count is read back to size the result."""
    lib = _lib.load()
    t, t0, t1, rad, nms, max_factors = int(t), int(t0), int(t1), int(rad), int(nms), int(max_factors)
    if (known_ii is None) != (known_jj is None):
        raise RuntimeError("proximity_edges: known_ii and known_jj go together")
    lists = [(sup_ii, "sup_ii", I64), (sup_jj, "sup_jj", I64)]
    if known_ii is not None:
        lists += [(known_ii, "known_ii", I64), (known_jj, "known_jj", I64)]
    if dist is None:
        check_tensors("proximity_edges", lists + _state(poses, disps, intrinsics))
        dist = frame_distance_matrix(poses, disps, intrinsics, t, beta, bidirectional=False)
    else:
        check_tensors("proximity_edges", lists)
        if dist.dtype != torch.float32 or dist.dim() != 2 or (dist.numel() and dist.stride(1) != 1):
            raise RuntimeError("proximity_edges: dist must be a float32 matrix with unit column stride")
        if dist.shape[0] < t or dist.shape[1] < t:
            raise RuntimeError("proximity_edges: dist is smaller than [t, t]")
        check_tensors("proximity_edges", [(dist, "dist", None)], types=False, contiguous=False)   # rows may be padded
    dev = dist.device
    n_sup, n_known = int(sup_ii.shape[0]), 0 if known_ii is None else int(known_ii.shape[0])
    if int(sup_jj.shape[0]) != n_sup or (n_known and int(known_jj.shape[0]) != n_known):
        raise RuntimeError("proximity_edges: ii and jj of an edge list must have one length")
    cap = proximity_edge_bound(t, t0, t1, rad, max_factors, bool(stereo))
    nbytes = lib.droid_proximity_workspace_bytes(t, t0, t1, n_known, cap)
    ws = _prox_ws.get_bytes(_ws_key(dev), nbytes, dev)
    out = torch.empty((cap, 2), dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ld = int(dist.stride(0)) if dist.shape[0] > 1 else max(int(dist.shape[1]), t)
    _lib.check(lib.droid_proximity_edges(
        _ptr(dist) or None, ld, 1, t, t0, t1, rad, nms, float(thresh), max_factors, int(bool(stereo)),
        _ptr(sup_ii) if n_sup else None, _ptr(sup_jj) if n_sup else None, n_sup,
        _ptr(known_ii) if n_known else None, _ptr(known_jj) if n_known else None, n_known,
        out.data_ptr() if cap else None, cap, count.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "proximity_edges")
    n = int(count.item())   # the one synchronisation (the reference's torch.as_tensor(es) is one too)
    return out[:n, 0], out[:n, 1]


def projmap(poses, disps, intrinsics, ii, jj):
    """droid.cpp:139-154 -> projmap_cuda droid_kernels.cu:1463-1488."""
    lib = _lib.load()
    check_tensors("projmap", _state(poses, disps, intrinsics) + [(ii, "ii", I64), (jj, "jj", I64)])
    nbuf, H, W = disps.shape
    nbuf = min(int(nbuf), int(poses.shape[0]))
    E = int(ii.shape[0])
    coords = torch.empty((E, H, W, 3), dtype=torch.float32, device=poses.device)
    valid = torch.empty((E, H, W, 1), dtype=torch.float32, device=poses.device)
    _lib.check(lib.droid_projmap(poses.data_ptr(), disps.data_ptr(), intrinsics.data_ptr(), ii.data_ptr(),
                                 jj.data_ptr(), E, nbuf, H, W, coords.data_ptr(), valid.data_ptr(),
                                 _stream()), "projmap")
    return [coords, valid]


def reproject(poses, disps, intrinsics, ii, jj, target=None):
    """`DepthVideo.reproject` (droid_slam/depth_video.py:150-158 -> geom/projective_ops.py:96-125) without
    lietorch: coords [1,E,H,W,2], valid [1,E,H,W,1] for the edges ii -> jj; stereo edges (ii == jj) use the fixed
    baseline.  `intrinsics` is [nbuf,4] (per frame, as `video.intrinsics`) or [4].  With `target` [1,E,H,W,2]
    (or [E,H,W,2]) the motion features of factor_graph.py:203-205 are produced in the same pass and returned as
    a third tensor [1,E,4,H,W]."""
    lib = _lib.load()
    check_tensors("reproject", _state(poses, disps, intrinsics) + [(ii, "ii", I64), (jj, "jj", I64)]
                  + ([(target, "target", F32)] if target is not None else []))
    if poses.dim() == 3:  # accept the batched [1,nbuf,...] tensors the caller holds
        poses, disps = poses[0], disps[0]
        if intrinsics.dim() == 3:
            intrinsics = intrinsics[0]
    poses, disps, intrinsics = poses.contiguous(), disps.contiguous(), intrinsics.contiguous()
    ii, jj = ii.reshape(-1).contiguous(), jj.reshape(-1).contiguous()
    nbuf, H, W = disps.shape
    nbuf = min(int(nbuf), int(poses.shape[0]))
    stride = 4 if intrinsics.dim() == 2 else 0
    if stride == 4 and int(intrinsics.shape[0]) < nbuf:
        raise ValueError("reproject: intrinsics has fewer rows than frames")
    E = int(ii.shape[0])
    coords = torch.empty((1, E, H, W, 2), dtype=torch.float32, device=poses.device)
    valid = torch.empty((1, E, H, W, 1), dtype=torch.float32, device=poses.device)
    motn = None
    tptr = None
    if target is not None:
        target = target.reshape(E, H, W, 2).contiguous()
        motn = torch.empty((1, E, 4, H, W), dtype=torch.float32, device=poses.device)
        tptr = target.data_ptr()
    _lib.check(lib.droid_reproject_motion(poses.data_ptr(), disps.data_ptr(), intrinsics.data_ptr(), stride,
                                          ii.data_ptr(), jj.data_ptr(), tptr, E, nbuf, H, W, coords.data_ptr(),
                                          valid.data_ptr(), motn.data_ptr() if motn is not None else None,
                                          _stream()), "reproject")
    return (coords, valid) if motn is None else (coords, valid, motn)


def motion_features(poses, disps, intrinsics, ii, jj, target):
    """factor_graph.py:203-205 in one call: `coords1, mask = video.reproject(ii, jj);
    motn = cat([coords1 - coords0, target - coords1], -1).permute(0,1,4,2,3).clamp(-64, 64)` -> (motn, coords1, mask)."""
    coords, valid, motn = reproject(poses, disps, intrinsics, ii, jj, target)
    return motn, coords, valid


def depth_filter(poses, disps, intrinsics, ix, thresh):
    """droid.cpp:220-234 -> depth_filter_cuda droid_kernels.cu:1491-1515."""
    lib = _lib.load()
    check_tensors("depth_filter", _state(poses, disps, intrinsics) + [(thresh, "thresh", F32), (ix, "ix", I64)])
    nbuf, H, W = disps.shape
    nbuf = min(int(nbuf), int(poses.shape[0]))
    num = int(ix.shape[0])
    counter = torch.empty((num, H, W), dtype=torch.float32, device=disps.device)
    _lib.check(lib.droid_depth_filter(poses.data_ptr(), disps.data_ptr(), intrinsics.data_ptr(), ix.data_ptr(),
                                      thresh.data_ptr(), num, nbuf, H, W, counter.data_ptr(), _stream()),
               "depth_filter")
    return counter


def iproj(poses, disps, intrinsics):
    """droid.cpp:157-166 -> iproj_cuda droid_kernels.cu:1518-1541."""
    lib = _lib.load()
    check_tensors("iproj", _state(poses, disps, intrinsics))
    nm, H, W = disps.shape
    points = torch.empty((nm, H, W, 3), dtype=torch.float32, device=disps.device)
    _lib.check(lib.droid_iproj(poses.data_ptr(), disps.data_ptr(), intrinsics.data_ptr(), nm, H, W,
                               points.data_ptr(), _stream()), "iproj")
    return points


_pc_ws = ScratchCache()   # _ws_key(device) -> grow-only uint8 scratch of point_cloud


class PointCloud:
    """What `point_cloud` returns: points [P,3] float32, colors [P,3] float32 or None, src [P] int32 (pixel v * w + u),
    offsets [n+1] int32 on the device (selection b owns rows offsets[b]:offsets[b+1]), matrices [n,4,4] float32, and
    offsets_host, the same offsets as a list of ints (None with sync=False, where the tensors keep their capacity
    n * h * w and rows from offsets[n] on are unwritten)."""
    __slots__ = ("points", "colors", "src", "offsets", "matrices", "offsets_host")

    def __init__(self, points, colors, src, offsets, matrices, offsets_host):
        self.points, self.colors, self.src = points, colors, src
        self.offsets, self.matrices, self.offsets_host = offsets, matrices, offsets_host

    def __len__(self):
        if self.offsets_host is None:
            raise TypeError("len() of a point cloud that was not synchronised (sync=False): read offsets[-1]")
        return self.offsets_host[-1]


def point_cloud(poses, disps, intrinsics, index, thresh, images=None, min_count=2, disp_ratio=0.5, sync=True):
    """The filtered, coloured point cloud of the keyframes `index` -- the body of the reference fork's viewers
    (visualization.py:100-142: SE3(poses).inv(), iproj, depth_filter, `(count >= 2) & (disps > .5 * mean)`, the colour
    lookup `images[:, [2,1,0], 3::8, 3::8] / 255.0` and the per-frame boolean indexing) in one call, with nothing per
    pixel on the host.  poses [nbuf,7], disps [nbuf,h,w], intrinsics [4] float32; index [n] int64 on the device (never
    read by the host; an entry outside the buffer yields no point and a zero matrix); thresh a Python float or an [n]
    float32 tensor, one per selection; images [nbuf,3,8h,8w] uint8 (BGR, as `video.images`) or None.  Returns a
    `PointCloud`: the points in the order of index, row-major within a frame.  sync=True reads offsets (n + 1
    integers, the one synchronisation) and trims points / colors / src to the P points kept; sync=False reads nothing
    and returns the capacity tensors [n * h * w, ...].  Contract: include/droid_backends_hip.h (droid_point_cloud).
    No autograd.  An addition."""
    lib = _lib.load()
    what = "point_cloud"
    tensors = _state(poses, disps, intrinsics) + [(index, "index", I64)]
    if isinstance(thresh, torch.Tensor):
        tensors.append((thresh, "thresh", F32))
    if images is not None:
        tensors.append((images, "images", torch.uint8))
    check_tensors(what, tensors, placement=False)
    if poses.dim() != 2 or poses.shape[1] != 7 or disps.dim() != 3 or intrinsics.dim() != 1 or intrinsics.shape[0] != 4:
        raise RuntimeError(f"{what}: poses must be [nbuf, 7], disps [nbuf, h, w], intrinsics [4], got "
                           f"{tuple(poses.shape)}, {tuple(disps.shape)}, {tuple(intrinsics.shape)}")
    if index.dim() != 1:
        raise RuntimeError(f"{what}: index must be [n], got {tuple(index.shape)}")
    n = int(index.shape[0])
    nbuf, h, w = (int(v) for v in disps.shape)
    if isinstance(thresh, torch.Tensor) and tuple(thresh.shape) != (n,):
        raise RuntimeError(f"{what}: thresh must be a number or [n] = [{n}], one per selection, got {tuple(thresh.shape)}")
    if images is not None and tuple(images.shape) != (nbuf, 3, 8 * h, 8 * w):
        raise RuntimeError(f"{what}: images must be [{nbuf}, 3, {8 * h}, {8 * w}] for {nbuf} frames of {h} x {w}, got "
                           f"{tuple(images.shape)}")
    check_tensors(what, tensors, types=False, on=(disps, "disps"))
    if h < 1 or w < 1:
        raise RuntimeError(f"{what}: disps must have h, w >= 1, got {tuple(disps.shape)}")
    if n * h * w >= 2 ** 31:
        raise RuntimeError(f"{what}: n * h * w = {n * h * w} reaches 2^31 (rows and offsets are 32-bit): select in parts")
    dev = disps.device
    nbuf = min(nbuf, int(poses.shape[0]))
    with torch.cuda.device(dev):
        if not isinstance(thresh, torch.Tensor):
            thresh = torch.full((n,), float(thresh), dtype=torch.float32, device=dev)
        cap = n * h * w
        points = torch.empty((cap, 3), dtype=torch.float32, device=dev)
        colors = torch.empty((cap, 3), dtype=torch.float32, device=dev) if images is not None else None
        src = torch.empty((cap,), dtype=torch.int32, device=dev)
        matrices = torch.empty((n, 4, 4), dtype=torch.float32, device=dev)
        if n == 0 or nbuf == 0:   # nothing selected (or nothing to select from): no launch
            offsets = torch.zeros((n + 1,), dtype=torch.int32, device=dev)
            matrices.zero_()
            return PointCloud(points[:0], None if colors is None else colors[:0], src[:0], offsets, matrices,
                              [0] * (n + 1) if sync else None)
        offsets = torch.empty((n + 1,), dtype=torch.int32, device=dev)
        stream = _stream()
        ws = _pc_ws.get_bytes(_ws_key(dev), lib.droid_point_cloud_workspace_bytes(n, h, w), dev)
        _lib.check(lib.droid_point_cloud(poses.data_ptr(), disps.data_ptr(), intrinsics.data_ptr(), index.data_ptr(),
                                         thresh.data_ptr(), _ptr(images), n, nbuf, h, w, int(min_count), float(disp_ratio),
                                         points.data_ptr(), _ptr(colors), src.data_ptr(), offsets.data_ptr(),
                                         matrices.data_ptr(), ws.data_ptr(), ws.numel(), stream), what)
        if not sync:
            return PointCloud(points, colors, src, offsets, matrices, None)
        host = offsets.tolist()   # the one synchronisation: n + 1 integers
    P = host[-1]
    return PointCloud(points[:P], None if colors is None else colors[:P], src[:P], offsets, matrices, host)


def _upsample_args(what, mask, n, h, w, f32, ix=None):
    """Checks of a convex upsampling, shapes and dtypes before devices so that a caller's mistake is named as what it
    is: f32 = ((tensor, name), ...) must be contiguous float32; the mask is returned as [n, 576, h, w], half or fp32
    (droid_cvx_upsample); every tensor must be on one HIP device."""
    if mask.dim() == 5 and mask.shape[0] == 1:
        mask = mask[0]
    tensors = ([(x, name, F32) for x, name in f32] + ([(ix, "ix", I64)] if ix is not None else [])
               + [(mask, "mask", F16_OR_F32)])
    check_tensors(what, tensors, placement=False)
    if mask.dim() != 4 or mask.shape[-3] != 576:
        raise RuntimeError(f"{what}: mask must be [1, n, 576, h, w] or [n, 576, h, w] (9 taps x 8 x 8 sub-pixels), got "
                           f"{tuple(mask.shape)}")
    if tuple(mask.shape) != (n, 576, h, w):
        raise RuntimeError(f"{what}: mask must be [{n}, 576, {h}, {w}] for {n} frames of {h} x {w}, got {tuple(mask.shape)}")
    check_tensors(what, tensors, types=False, on=(mask, "the mask"))
    return mask


def upsample_disps(disps, ix, mask, out):
    """The body of `DepthVideo.upsample` (droid_slam/depth_video.py:134-138) in one launch:
    out[ix] = cvx_upsample(disps[ix].unsqueeze(-1), mask).squeeze(-1), without the gathered copy, the fp32 product
    [n, 1, 9, 8, 8, h, w], the permuted copy and the index_put.  disps [buffer, h, w] float32 (only read); ix [n] int64
    on the device, pairwise distinct; mask [1, n, 576, h, w] or [n, 576, h, w], float16 or float32 (the update
    operator's `upmask`); out [buffer, 8h, 8w] float32, written in place at the frames ix and returned.  A frame index
    outside both buffers is skipped.  The softmax weights stay fp32 (the stock chain rounds them to half for a half
    mask).  Never synchronises; no autograd.  Contract: include/droid_backends_hip.h (droid_cvx_upsample).  An addition."""
    lib = _lib.load()
    if disps.dim() != 3 or out.dim() != 3 or ix.dim() != 1:
        raise RuntimeError("upsample_disps: disps must be [buffer, h, w], out [buffer, 8h, 8w], ix [n]")
    nbuf_in, h, w = (int(v) for v in disps.shape)
    if tuple(out.shape[1:]) != (8 * h, 8 * w):
        raise RuntimeError(f"upsample_disps: out must be [buffer, {8 * h}, {8 * w}], got {tuple(out.shape)}")
    n = int(ix.shape[0])
    mask = _upsample_args("upsample_disps", mask, n, h, w, ((disps, "disps"), (out, "out")), ix)
    _lib.check(lib.droid_cvx_upsample(disps.data_ptr(), ix.data_ptr(), mask.data_ptr(), out.data_ptr(), n, nbuf_in,
                                      int(out.shape[0]), h, w, _DT[mask.dtype], _stream()), "upsample_disps")
    return out


def cvx_upsample(data, mask):
    """Drop-in for `droid_net.cvx_upsample` (droid_net.py:21-35) in the one form the reference calls it with:
    data [batch, ht, wd, 1] float32, mask anything that views to [batch, 576, ht, wd] (float16 or float32).  Returns a
    new [batch, 8 ht, 8 wd, 1] float32 tensor (droid_cvx_upsample with ix = NULL).  Inference only: no autograd."""
    lib = _lib.load()
    if data.dim() != 4 or data.shape[-1] != 1:
        raise RuntimeError(f"cvx_upsample: data must be [batch, ht, wd, 1] -- only dim = 1 (a disparity map) is "
                           f"supported, got {tuple(data.shape)}")
    if torch.is_grad_enabled() and (data.requires_grad or mask.requires_grad):
        raise RuntimeError("cvx_upsample: no autograd -- training keeps the stock droid_net.cvx_upsample")
    batch, ht, wd = (int(v) for v in data.shape[:3])
    if not mask.is_contiguous():
        raise RuntimeError("cvx_upsample: mask must be contiguous")
    if mask.numel() != batch * 576 * ht * wd:
        raise RuntimeError(f"cvx_upsample: mask must view to [{batch}, 576, {ht}, {wd}], got {tuple(mask.shape)}")
    mask = _upsample_args("cvx_upsample", mask.view(batch, 576, ht, wd), batch, ht, wd, ((data, "data"),))
    out = torch.empty((batch, 8 * ht, 8 * wd, 1), dtype=torch.float32, device=data.device)
    _lib.check(lib.droid_cvx_upsample(data.data_ptr(), None, mask.data_ptr(), out.data_ptr(), batch, batch, batch, ht, wd,
                                      _DT[mask.dtype], _stream()), "cvx_upsample")
    return out


_gm_ws = ScratchCache()   # _ws_key(device) -> grow-only uint8 scratch of graph_mean / scatter_mean


def _graph_mean_args(what, src, index, batched):
    """The checks both entry points share, a caller's mistake named before the device is looked at.  Returns src as
    [E, ...] rows (src[0] when `batched`: [1, E, ...])."""
    tensors = [(src, "src", F16_OR_F32), (index, "index", I64)]
    check_tensors(what, tensors, placement=False)
    if torch.is_grad_enabled() and src.requires_grad:
        raise RuntimeError(f"{what}: no autograd -- training keeps torch_scatter (inference only)")
    if batched and src.shape[0] != 1:
        raise RuntimeError(f"{what}: batch must be 1, got {int(src.shape[0])}")
    rows = src[0] if batched else src
    if index.dim() != 1 or int(index.shape[0]) != int(rows.shape[0]):
        raise RuntimeError(f"{what}: index must be [E] = [{int(rows.shape[0])}], one group per row of src, got "
                           f"{tuple(index.shape)}")
    check_tensors(what, tensors, types=False, on=(src, "src"))
    return rows


def _graph_mean_run(what, rows, batched, index, M, rng, compact):
    lib = _lib.load()
    dev = rows.device
    E = int(rows.shape[0])
    out = torch.empty(((1,) if batched else ()) + (M,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=dev)
    plane = 1
    for v in rows.shape[1:]:
        plane *= int(v)
    if M == 0 or plane == 0:
        return out
    ws, stream = None, _stream()
    if E > 0:
        nbytes = lib.droid_graph_mean_workspace_bytes(E, rng)   # 0 for sizes the call below refuses by name
        ws = _gm_ws.get_bytes(_ws_key(dev), nbytes, dev)
    _lib.check(lib.droid_graph_mean(rows.data_ptr() if E else None, index.data_ptr() if E else None, out.data_ptr(),
                                    E, plane, M, rng, compact, _DT[rows.dtype], None, _ptr(ws),
                                    ws.numel() if ws is not None else 0, stream), what)
    return out


def graph_mean(net, ii, num_groups=None, nbuf=None):
    """`GraphAgg.forward`'s source-frame mean (droid_slam/droid_net.py:63-67) with its `torch.unique` fused:
    `_, ix = torch.unique(ii, return_inverse=True); net = scatter_mean(net, ix, dim=1)` becomes
    `net = graph_mean(net, ii)`.  net [1, E, C, H, W] or [E, C, H, W], float16 or float32, contiguous; ii [E] int64.
    Returns [1, M, C, H, W] or [M, C, H, W]: row g is the mean over the edges whose source is the g-th smallest distinct
    frame.  M = num_groups when given (then the host reads nothing; rows beyond the distinct count are +0.0), else
    torch.unique(ii).numel(), the reference's own synchronisation.  nbuf = the frame-buffer size (frames outside
    [0, nbuf) are ignored); None reads int(ii.max()) + 1.  fp32 sums in edge order, no atomics: the same bits on every
    run.  Contract: include/droid_backends_hip.h (droid_graph_mean, compact = 1).  Inference only.  An addition."""
    if net.dim() not in (4, 5):
        raise RuntimeError(f"graph_mean: net must be [1, E, C, H, W] or [E, C, H, W], got {tuple(net.shape)}")
    batched = net.dim() == 5
    rows = _graph_mean_args("graph_mean", net, ii, batched)
    E = int(ii.shape[0])
    rng = int(nbuf) if nbuf is not None else (int(ii.max()) + 1 if E else 1)
    M = int(num_groups) if num_groups is not None else int(torch.unique(ii).numel())
    if M < 0:
        raise RuntimeError("graph_mean: num_groups must not be negative")
    return _graph_mean_run("graph_mean", rows, batched, ii, M, max(rng, 1), 1)


def scatter_mean(src, index, dim=1, dim_size=None):
    """`torch_scatter.scatter_mean(src, index, dim=1)` in the one form `GraphAgg` calls it with
    (`from droid_backends import scatter_mean` replaces the import): src [1, E, ...] with dim = 1, or [E, ...] with
    dim = 0, float16 or float32, contiguous; index [E] int64.  Row r of the result is the mean of the entries with
    index == r, a row without entries +0.0; rows = dim_size, or int(index.max()) + 1 (the read torch_scatter makes too).
    Entries outside [0, rows) are ignored.  Contract: include/droid_backends_hip.h (droid_graph_mean, compact = 0).
    Inference only: no autograd."""
    if dim not in (0, 1) or src.dim() < dim + 1:
        raise RuntimeError(f"scatter_mean: only dim = 1 on [1, E, ...] or dim = 0 on [E, ...] is supported, got dim = "
                           f"{dim} on {tuple(src.shape)}")
    rows = _graph_mean_args("scatter_mean", src, index, dim == 1)
    M = int(dim_size) if dim_size is not None else (int(index.max()) + 1 if index.numel() else 0)
    if M < 0:
        raise RuntimeError("scatter_mean: dim_size must not be negative")
    return _graph_mean_run("scatter_mean", rows, dim == 1, index, M, max(M, 1), 0)


def _corr_dtype(t, name):
    if t.dtype not in _DT:
        raise RuntimeError(f"{name}: unsupported dtype {t.dtype} (float16/float32/float64)")
    return _DT[t.dtype]


def corr_index_forward(volume, coords, radius):
    """droid.cpp:170-178 -> corr_index_cuda_forward correlation_kernels.cu:126-155."""
    lib = _lib.load()
    check_tensors("corr_index_forward", [(volume, "volume", None), (coords, "coords", F32)])
    B, H1, W1, H2, W2 = volume.shape
    r = int(radius)
    corr = torch.empty((B, 2 * r + 1, 2 * r + 1, H1, W1), dtype=volume.dtype, device=volume.device)
    _lib.check(lib.droid_corr_index_forward(volume.data_ptr(), coords.data_ptr(), corr.data_ptr(), B, H1, W1,
                                            H2, W2, r, _corr_dtype(volume, "volume"), _stream()),
               "corr_index_forward")
    return [corr]


def corr_pyramid_forward(pyramid, coords, radius, slots=None):
    """CorrBlock.__call__ (droid_slam/modules/corr.py:40-50) without the torch.cat: pyramid = CorrBlock.corr_pyramid
    (list of [B,h,w,h>>l,w>>l] volumes of one dtype), coords [B,2,h,w] float32 at level-0 scale (the tensor __call__
    builds at :43-44).  Returns [corr] with corr [B, levels*(2r+1)^2, h, w] = torch.cat([corr_index_forward(
    pyramid[l], coords / 2**l, r).view(B, -1, h, w) for l], dim=1), bit for bit.  An addition.
    With `slots` ([B] int64 on the device) the pyramid is a list of capacity buffers [cap,h,w,h>>l,w>>l] and entry b
    reads slot slots[b]: the result of corr_pyramid_forward([p[slots] for p in pyramid], coords, radius) bit for bit,
    without the gathered copy; a slot outside [0, cap) gives zeros for that entry (droid_corr_pyramid_forward_slots)."""
    lib = _lib.load()
    levels = list(pyramid)
    check_tensors("corr_pyramid_forward", [(p, f"pyramid[{i}]", None) for i, p in enumerate(levels)]
                  + [(coords, "coords", F32)] + ([(slots, "slots", I64)] if slots is not None else []))
    if any(p.dtype != levels[0].dtype for p in levels):
        raise RuntimeError("corr_pyramid_forward: pyramid levels must share one dtype")
    cap, H1, W1 = int(levels[0].shape[0]), int(levels[0].shape[1]), int(levels[0].shape[2])
    for l, p in enumerate(levels):
        if tuple(p.shape) != (cap, H1, W1, H1 >> l, W1 >> l):
            raise RuntimeError(f"corr_pyramid_forward: pyramid[{l}] must be [{cap},{H1},{W1},{H1 >> l},{W1 >> l}]")
    B = cap
    if slots is not None:
        if slots.dim() != 1:
            raise RuntimeError("corr_pyramid_forward: slots must be [B]")
        B = int(slots.shape[0])
    if tuple(coords.shape) != (B, 2, H1, W1):
        raise RuntimeError("corr_pyramid_forward: coords must be [B,2,H1,W1]")
    r = int(radius)
    rd2 = (2 * r + 1) ** 2
    corr = torch.empty((B, len(levels) * rd2, H1, W1), dtype=levels[0].dtype, device=levels[0].device)
    ptrs = (ctypes.c_void_p * len(levels))(*[p.data_ptr() for p in levels])
    if slots is None:
        _lib.check(lib.droid_corr_pyramid_forward(ptrs, coords.data_ptr(), corr.data_ptr(), B, H1, W1, r, len(levels),
                                                  _corr_dtype(levels[0], "pyramid"), _stream()), "corr_pyramid_forward")
    else:
        _lib.check(lib.droid_corr_pyramid_forward_slots(ptrs, slots.data_ptr(), coords.data_ptr(), corr.data_ptr(), B, cap,
                                                        H1, W1, r, len(levels), _corr_dtype(levels[0], "pyramid"),
                                                        _stream()), "corr_pyramid_forward")
    return [corr]


def corr_volume_pyramid(fmaps, ii, jj, levels=4, out=None, offset=0, slots=None):
    """CorrBlock.__init__ (droid_slam/modules/corr.py:24-38, 63-71) for the edges ii -> jj in one launch, from the
    feature buffer as DepthVideo holds it: fmaps [nbuf, ncam, C, h, w] (or [nbuf, C, h, w]) float16 / float32, channels
    first; ii, jj [E] int64.  Edge e correlates fmaps[ii[e], 0] / 4 with fmaps[jj[e], c] / 4, c = 1 for a stereo edge
    (ncam == 2 and ii[e] == jj[e]), and pools level l+1 from the rounded level l like avg_pool2d; an index outside
    [0, nbuf) yields zeros.  Returns the list CorrBlock.corr_pyramid: level l = [E, h, w, h>>l, w>>l] of fmaps' dtype.
    With `out` (a list of capacity tensors [cap, h, w, h>>l, w>>l]) the edges are written to slots
    [offset, offset + E) -- every other slot is left as it is -- and views of those slots are returned: allocate the
    pyramid once and build new edges at offset = number of edges held, instead of CorrBlock.cat.
    With `out` and `slots` ([E] int64 on the device, pairwise distinct) edge e is written to slot slots[e] instead, an
    edge whose slot is outside [0, cap) is skipped, and `out` itself is returned (droid_corr_volume_pyramid_slots).
    The contract is in include/droid_backends_hip.h (droid_corr_volume_pyramid).  An addition."""
    lib = _lib.load()
    check_tensors("corr_volume_pyramid", [(fmaps, "fmaps", F16_OR_F32), (ii, "ii", I64), (jj, "jj", I64)]
                  + ([(slots, "slots", I64)] if slots is not None else []))
    if fmaps.dim() == 4:
        fmaps = fmaps[:, None]
    if fmaps.dim() != 5:
        raise RuntimeError("corr_volume_pyramid: fmaps must be [nbuf, ncam, C, h, w] or [nbuf, C, h, w]")
    nbuf, ncam, C, h, w = (int(x) for x in fmaps.shape)
    levels, offset = int(levels), int(offset)
    if ii.dim() != 1 or ii.shape != jj.shape:
        raise RuntimeError("corr_volume_pyramid: ii and jj must be [E]")
    E = int(ii.shape[0])
    shapes = [(h, w, h >> l, w >> l) for l in range(levels)]
    given_out = out is not None
    if out is None:
        if offset != 0:
            raise RuntimeError("corr_volume_pyramid: offset needs out")
        out = [torch.empty((E,) + s, dtype=fmaps.dtype, device=fmaps.device) for s in shapes]
    else:
        out = list(out)
        if len(out) != levels:
            raise RuntimeError(f"corr_volume_pyramid: out must hold {levels} levels")
        check_tensors("corr_volume_pyramid", [(o, f"out[{l}]", None) for l, o in enumerate(out)])
        for l, o in enumerate(out):
            if o.dtype != fmaps.dtype or o.dim() != 5 or tuple(o.shape[1:]) != shapes[l] or o.shape[0] != out[0].shape[0]:
                raise RuntimeError(f"corr_volume_pyramid: out[{l}] must be [cap,{h},{w},{h >> l},{w >> l}] of {fmaps.dtype}")
    cap = int(out[0].shape[0]) if levels > 0 else 0
    if slots is not None:
        if not given_out:
            raise RuntimeError("corr_volume_pyramid: slots needs out")
        if offset != 0:
            raise RuntimeError("corr_volume_pyramid: slots and offset exclude each other")
        if tuple(slots.shape) != (E,):
            raise RuntimeError("corr_volume_pyramid: slots must be [E]")
        ptrs = (ctypes.c_void_p * max(levels, 1))(*[o.data_ptr() for o in out])
        _lib.check(lib.droid_corr_volume_pyramid_slots(fmaps.data_ptr(), ii.data_ptr(), jj.data_ptr(), ptrs,
                                                       slots.data_ptr(), E, nbuf, ncam, C, h, w, levels, cap,
                                                       _DT[fmaps.dtype], _stream()), "corr_volume_pyramid")
        return out
    if offset < 0 or offset + E > cap:
        raise RuntimeError(f"corr_volume_pyramid: slots [{offset}, {offset + E}) do not fit the capacity {cap}")
    ptrs = (ctypes.c_void_p * max(levels, 1))(*[o.data_ptr() for o in out])
    _lib.check(lib.droid_corr_volume_pyramid(fmaps.data_ptr(), ii.data_ptr(), jj.data_ptr(), ptrs, E, nbuf, ncam, C, h,
                                             w, levels, offset, cap, _DT[fmaps.dtype], _stream()), "corr_volume_pyramid")
    return [o[offset:offset + E] for o in out]


def corr_index_backward(volume, coords, corr_grad, radius):
    """droid.cpp:180-191 -> corr_index_cuda_backward correlation_kernels.cu:157-185."""
    lib = _lib.load()
    check_tensors("corr_index_backward", [(volume, "volume", None), (coords, "coords", F32), (corr_grad, "corr_grad", None)])
    B, H1, W1, H2, W2 = volume.shape
    if corr_grad.dtype != volume.dtype:
        corr_grad = corr_grad.to(volume.dtype)
    volume_grad = torch.empty_like(volume)
    _lib.check(lib.droid_corr_index_backward(coords.data_ptr(), corr_grad.data_ptr(), volume_grad.data_ptr(), B,
                                             H1, W1, H2, W2, int(radius), _corr_dtype(volume, "volume"),
                                             _stream()), "corr_index_backward")
    return [volume_grad]


def altcorr_forward(fmap1, fmap2, coords, radius):
    """droid.cpp:193-203 -> altcorr_cuda_forward altcorr_kernel.cu:290-319."""
    lib = _lib.load()
    check_tensors("altcorr_forward", [(fmap1, "fmap1", None), (fmap2, "fmap2", None), (coords, "coords", None)])
    if fmap2.dtype != fmap1.dtype or coords.dtype != torch.float32:
        raise RuntimeError("altcorr_forward: fmap dtypes must match and coords must be float32")
    B, N, H, W, _ = coords.shape
    _, H1, W1, C = fmap1.shape
    _, H2, W2, _ = fmap2.shape
    r = int(radius)
    rd = 2 * r + 1
    corr = torch.empty((B, N, rd * rd, H, W), dtype=fmap1.dtype, device=fmap1.device)
    _lib.check(lib.droid_altcorr_forward(fmap1.data_ptr(), fmap2.data_ptr(), coords.data_ptr(), corr.data_ptr(),
                                         B, N, H1, W1, H2, W2, C, r, _corr_dtype(fmap1, "fmap1"), _stream()),
               "altcorr_forward")
    return [corr]


def altcorr_pyramid_forward(pyramid, coords, ii, jj, radius):
    """AltCorrBlock.corr_fn (droid_slam/modules/corr.py:105-125) in one launch, without the per-edge
    copies `pyramid[i][:, jj]`: pyramid = AltCorrBlock.pyramid (list of [1, frames, H>>l, W>>l, C]
    or [frames, ...] tensors), coords [E, H, W, 2] (or [1, E, H, W, 2]) float32 at level-0
    scale, ii / jj [E] int64.  Returns [corr] with corr [E, levels*(2r+1)^2, H, W] float32 =
    torch.cat([altcorr_forward(pyramid[0][ii].float(), pyramid[l][jj].float(), coords / 2**l, r) for l], dim=1).
    The pyramid may be float32 or -- what the SLAM path holds, `video.fmaps` is half (depth_video.py:44,
    factor_graph.py:260-261, modules/corr.py:97-104) -- float16: the half pyramid goes to the f16 matrix cores
    as it is (no `.float()` copies; the result is the fp32 evaluation of the widened maps up to summation order).
    Not one of the reference's nine operators."""
    lib = _lib.load()
    levels = [p[0] if p.dim() == 5 else p for p in pyramid]
    if coords.dim() == 5:
        coords = coords[0]
    check_tensors("altcorr_pyramid_forward", [(p, f"pyramid[{i}]", None) for i, p in enumerate(levels)]
                  + [(coords, "coords", None), (ii, "ii", None), (jj, "jj", None)])
    if any(p.dtype != levels[0].dtype or p.dtype not in F16_OR_F32 for p in levels):
        raise RuntimeError("altcorr_pyramid_forward: pyramid levels must all be float32 or all float16")
    if coords.dtype != torch.float32 or ii.dtype != torch.int64 or jj.dtype != torch.int64:
        raise RuntimeError("altcorr_pyramid_forward: coords must be float32 and ii/jj int64")
    frames, H, W, C = levels[0].shape
    for l, p in enumerate(levels):
        if tuple(p.shape) != (frames, H >> l, W >> l, C):
            raise RuntimeError(f"altcorr_pyramid_forward: pyramid[{l}] must be [{frames},{H >> l},{W >> l},{C}]")
    E = int(ii.shape[0])
    if tuple(coords.shape) != (E, H, W, 2) or int(jj.shape[0]) != E:
        raise RuntimeError("altcorr_pyramid_forward: coords must be [E,H,W,2] and ii, jj [E]")
    r = int(radius)
    rd = 2 * r + 1
    corr = torch.empty((E, len(levels) * rd * rd, H, W), dtype=torch.float32, device=coords.device)
    ptrs = (ctypes.c_void_p * len(levels))(*[p.data_ptr() for p in levels])
    fn = lib.droid_altcorr_pyramid_forward_f16 if levels[0].dtype == torch.float16 else lib.droid_altcorr_pyramid_forward
    _lib.check(fn(ptrs, ii.data_ptr(), jj.data_ptr(), coords.data_ptr(), corr.data_ptr(), E, int(frames), int(H),
                  int(W), int(C), r, len(levels), _stream()), "altcorr_pyramid_forward")
    return [corr]


def altcorr_backward(fmap1, fmap2, coords, corr_grad, radius):
    """droid.cpp:205-217 -> altcorr_cuda_backward altcorr_kernel.cu:322-355 (fp32 only, like the reference)."""
    lib = _lib.load()
    check_tensors("altcorr_backward", [(fmap1, "fmap1", F32), (fmap2, "fmap2", F32), (coords, "coords", F32),
                                       (corr_grad, "corr_grad", F32)])
    B, N, H, W, _ = coords.shape
    _, H1, W1, C = fmap1.shape
    _, H2, W2, _ = fmap2.shape
    fmap1_grad = torch.zeros_like(fmap1)
    fmap2_grad = torch.zeros_like(fmap2)
    coords_grad = torch.zeros_like(coords)
    _lib.check(lib.droid_altcorr_backward(fmap1.data_ptr(), fmap2.data_ptr(), coords.data_ptr(),
                                          corr_grad.data_ptr(), fmap1_grad.data_ptr(), fmap2_grad.data_ptr(),
                                          B, N, H1, W1, H2, W2, C, int(radius), _stream()), "altcorr_backward")
    return [fmap1_grad, fmap2_grad, coords_grad]
