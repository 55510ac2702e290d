"""The SE3 pose algebra of the reference's inference path without lietorch: the subset `PoseTrajectoryFiller`, the
visualiser, `Droid.terminate` and the multi-session tooling use, on [..., 7] pose records (tx ty tz qx qy qz qw), and the
filler's bracket search + interpolation in one launch.  Thin calls into the C ABI (include/droid_backends_hip.h, "pose
algebra") on PyTorch's current HIP stream; all arithmetic is in the HIP library, fp64 from the float32 records, rounded
once.  Inference only: no autograd, no action on points (`droid_backends.reproject` / `iproj` own those), no Sim3 / SO3.
Parity with lietorch is unpinned (it cannot be built for this device): the yardstick is tests/se3_ref.py."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._args import _stream, check_tensors

__all__ = ["SE3", "cat", "interpolate"]

INV, LOG, EXP, MATRIX = 0, 1, 2, 3   # DROID_SE3_*
_WIDTH_OUT = {INV: 7, LOG: 6, EXP: 7, MATRIX: 16}


def _check_type(x, what, name, width):
    check_tensors(what, [(x, name, torch.float32)], placement=False)
    if x.dim() < 1 or x.shape[-1] != width:
        raise RuntimeError(f"{what}: {name} must be [..., {width}], got {tuple(x.shape)}")


def _check(x, what, name, width):
    """A caller's mistake is named before the device is looked at; records are made contiguous, not refused."""
    _check_type(x, what, name, width)
    check_tensors(what, [(x, name, None)], types=False, contiguous=False)


def _unary(x, op, what):
    lib = _lib.load()
    n = x.numel() // x.shape[-1]
    w = _WIDTH_OUT[op]
    out = torch.empty(tuple(x.shape[:-1]) + (w,), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.droid_se3_unary(x.data_ptr(), out.data_ptr(), n, op, _stream()), what)
    return out


class SE3:
    """`lietorch.SE3` for inference: wraps a [..., 7] float32 tensor (made contiguous if needed, otherwise not copied).
    `.data`, `.shape` (the batch shape), `.device`; `.inv()`, `.log()`, `SE3.exp(xi)`, `.matrix()`; `a * b` for equal
    batch shapes or with either side one record; indexing on the batch dimensions; `len`.  Every group operation needs a
    HIP tensor; only `SE3.Identity` may live on the host (motion_filter.py:55 builds it there)."""

    def __init__(self, data):
        if isinstance(data, SE3):
            data = data.data
        check_tensors("SE3", [(data, "data", torch.float32)], placement=False)
        if data.dim() < 1 or data.shape[-1] != 7:
            raise RuntimeError(f"SE3: data must be [..., 7] (tx ty tz qx qy qz qw), got {tuple(data.shape)}")
        self.data = data if data.is_contiguous() else data.contiguous()

    @classmethod
    def _wrap(cls, data):
        self = object.__new__(cls)
        self.data = data
        return self

    @staticmethod
    def Identity(*batch, device=None, dtype=torch.float32):
        """Identity records of the batch shape `batch` (ints or one tuple).  Pure torch; the host is allowed."""
        if len(batch) == 1 and isinstance(batch[0], (tuple, list, torch.Size)):
            batch = tuple(batch[0])
        data = torch.zeros(tuple(int(b) for b in batch) + (7,), dtype=dtype, device=device)
        data[..., 6] = 1
        return SE3._wrap(data)

    @staticmethod
    def exp(xi):
        """The exponential map of [..., 6] tangents (tau, phi)."""
        _check(xi, "SE3.exp", "xi", 6)
        return SE3._wrap(_unary(xi.contiguous(), EXP, "SE3.exp"))

    @property
    def shape(self):
        return self.data.shape[:-1]

    @property
    def device(self):
        return self.data.device

    def __len__(self):
        if self.data.dim() < 2:
            raise TypeError("len() of a single SE3 record")
        return int(self.data.shape[0])

    def __getitem__(self, index):
        if not isinstance(index, tuple):
            index = (index,)
        return SE3(self.data[index + (slice(None),)])   # the record dimension is never indexed

    def __repr__(self):
        return f"SE3({self.data!r})"

    def inv(self):
        _check(self.data, "SE3.inv", "data", 7)
        return SE3._wrap(_unary(self.data, INV, "SE3.inv"))

    def log(self):
        """[..., 6] tangents (tau, phi), |phi| <= pi."""
        _check(self.data, "SE3.log", "data", 7)
        return _unary(self.data, LOG, "SE3.log")

    def matrix(self):
        """[..., 4, 4], last row 0 0 0 1."""
        _check(self.data, "SE3.matrix", "data", 7)
        return _unary(self.data, MATRIX, "SE3.matrix").view(tuple(self.shape) + (4, 4))

    def __mul__(self, other):
        if not isinstance(other, SE3):
            raise TypeError("SE3 * " + type(other).__name__ + ": only SE3 * SE3 is provided; the actions on points are "
                            "droid_backends.reproject and droid_backends.iproj")
        a, b = self.data, other.data
        _check(a, "SE3.__mul__", "the left operand", 7)
        _check(b, "SE3.__mul__", "the right operand", 7)
        if a.device != b.device:
            raise RuntimeError(f"SE3.__mul__: operands are on {a.device} and {b.device}")
        na, nb = a.numel() // 7, b.numel() // 7
        if a.shape == b.shape:
            shape, sa, sb = a.shape, 7, 7
        elif nb == 1:
            shape, sa, sb = a.shape, 7, 0
        elif na == 1:
            shape, sa, sb = b.shape, 0, 7
        else:
            raise RuntimeError(f"SE3.__mul__: batch shapes {tuple(self.shape)} and {tuple(other.shape)} neither match nor "
                               f"hold a single record")
        out = torch.empty(shape, dtype=torch.float32, device=a.device)
        lib = _lib.load()
        with torch.cuda.device(a.device):
            _lib.check(lib.droid_se3_mul(a.data_ptr(), sa, b.data_ptr(), sb, out.data_ptr(), out.numel() // 7, _stream()),
                       "SE3.__mul__")
        return SE3._wrap(out)

    __rmul__ = None   # tensor * SE3 and number * SE3 are not group operations


def cat(poses, dim=0):
    """`lietorch.cat`: concatenate SE3 objects along the batch dimension `dim`."""
    poses = list(poses)
    if not poses or not all(isinstance(p, SE3) for p in poses):
        raise TypeError("cat: a non-empty list of SE3 objects is needed")
    nb = poses[0].data.dim() - 1
    if not -nb <= dim < nb:
        raise IndexError(f"cat: dim {dim} is not a batch dimension of {tuple(poses[0].shape)}")
    return SE3(torch.cat([p.data for p in poses], dim=dim if dim >= 0 else dim - 1))


def interpolate(poses, tstamp, n, query):
    """The interpolation of `PoseTrajectoryFiller.__fill` (droid_slam/trajectory_filler.py:44-58) in one launch:
    poses [>= n, 7] and tstamp [>= n] float32 on the device (`video.poses`, `video.tstamp`), n = `video.counter.value`,
    query = the stamps to fill (a list, a numpy array or a tensor of any real dtype; converted to float32 on the
    device).  Returns (SE3 [M], k0 [M] int64, k1 [M] int64): the poses `Gs`, and the brackets `t0`, `t1` that the
    filler hands to `add_factors`.  Never synchronises.  A query before every stamp clamps to the first bracket (the
    reference wraps to the last keyframe); contract: include/droid_backends_hip.h (droid_pose_interpolate)."""
    what = "pose_interpolate"
    if isinstance(poses, SE3):
        poses = poses.data
    _check_type(poses, what, "poses", 7)
    if not isinstance(tstamp, torch.Tensor) or tstamp.dtype != torch.float32:
        raise RuntimeError(f"{what}: tstamp must be a float32 tensor, got {getattr(tstamp, 'dtype', type(tstamp).__name__)}")
    if poses.dim() != 2 or tstamp.dim() != 1:
        raise RuntimeError(f"{what}: poses must be [buffer, 7] and tstamp [buffer], got {tuple(poses.shape)} and "
                           f"{tuple(tstamp.shape)}")
    check_tensors(what, [(poses, "poses", None), (tstamp, "tstamp", None)], types=False, contiguous=False, on=(poses, "poses"))
    n = int(n)
    if n < 1 or n > int(poses.shape[0]) or n > int(tstamp.shape[0]):
        raise RuntimeError(f"{what}: n = {n} must be at least 1 and at most the rows of poses and tstamp")
    dev = poses.device
    if isinstance(query, torch.Tensor):
        if query.is_complex() or query.dtype == torch.bool:
            raise RuntimeError(f"{what}: query must be real, got {query.dtype}")
        q = query.to(device=dev, dtype=torch.float32)
    else:
        q = torch.as_tensor(np.asarray(query, dtype=np.float32), device=dev)
    q = q.reshape(-1).contiguous()
    poses, tstamp = poses.contiguous(), tstamp.contiguous()
    M = int(q.shape[0])
    out = torch.empty((M, 7), dtype=torch.float32, device=dev)
    k = torch.empty((2, M), dtype=torch.int64, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.droid_pose_interpolate(poses.data_ptr(), tstamp.data_ptr(), n, q.data_ptr(), M, out.data_ptr(),
                                              k[0].data_ptr(), k[1].data_ptr(), _stream()), what)
    return SE3._wrap(out), k[0], k[1]
