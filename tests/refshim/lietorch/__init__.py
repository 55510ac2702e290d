"""Stand-in for the `lietorch` names the reference's Python programs use (tests/reference_programs.py puts this
directory on sys.path for the time of one `with` block, nowhere else).  Written from the semantics of the group, not
from lietorch: an element is a record (tx ty tz qx qy qz qw) on the last axis of `.data`, x -> R(q) x + t; tangents are
ordered (tau, phi).  Plain torch, dtype-preserving (the generator and the tests use float64), no autograd functions of
its own.  Pinned by tests/test_reference_pin.py: mul / inv / action / exp / retr against tests/se3_ref.py, adjT through
finite differences of the reference's own projection.

Only what geom/projective_ops.py, geom/ba.py and droid_net.py touch is here; `Sim3` and `SO3` exist as names only.
"""
import torch


def _rot(q, x):
    """R(q) x for q = (x y z w), broadcasting: x + w uv + v x uv with uv = 2 v x x."""
    v, w = q[..., :3], q[..., 3:4]
    v, x = torch.broadcast_tensors(v, x)
    uv = 2.0 * torch.linalg.cross(v, x)
    return x + w * uv + torch.linalg.cross(v, uv)


def _qmul(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw,
                        aw * bw - ax * bx - ay * by - az * bz], -1)


class SE3:
    manifold_dim = 6
    embedded_dim = 7

    def __init__(self, data):
        assert data.shape[-1] == 7, data.shape
        self.data = data

    # -- container behaviour ------------------------------------------------------------------------------------------
    @property
    def shape(self):
        return self.data.shape[:-1]

    @property
    def dtype(self):
        return self.data.dtype

    @property
    def device(self):
        return self.data.device

    def __getitem__(self, index):
        return SE3(self.data[index])

    def view(self, *shape):
        return SE3(self.data.view(*shape, 7))

    # -- the group ----------------------------------------------------------------------------------------------------
    @classmethod
    def exp(cls, xi):
        """(tau, phi) -> (V(phi) tau, q(phi)); the series below a squared angle of 1e-4 (next term < 1e-22 relative)."""
        tau, phi = xi[..., :3], xi[..., 3:]
        th2 = (phi * phi).sum(-1, keepdim=True)
        small = th2 < 1e-4
        th = torch.sqrt(torch.where(small, torch.ones_like(th2), th2))
        half = torch.where(small, 0.5 - th2 / 48 + th2 ** 2 / 3840 - th2 ** 3 / 645120, torch.sin(0.5 * th) / th)
        a = torch.where(small, 0.5 - th2 / 24 + th2 ** 2 / 720 - th2 ** 3 / 40320, (1 - torch.cos(th)) / th ** 2)
        b = torch.where(small, 1 / 6 - th2 / 120 + th2 ** 2 / 5040 - th2 ** 3 / 362880, (th - torch.sin(th)) / th ** 3)
        u = torch.linalg.cross(phi, tau)
        t = tau + a * u + b * torch.linalg.cross(phi, u)
        w = torch.cos(0.5 * torch.sqrt(th2))
        return cls(torch.cat([t, half * phi, w], -1))

    def inv(self):
        q = self.data[..., 3:] * self.data.new_tensor([-1.0, -1.0, -1.0, 1.0])
        return SE3(torch.cat([-_rot(q, self.data[..., :3]), q], -1))

    def __mul__(self, other):
        t, q = self.data[..., :3], self.data[..., 3:]
        if isinstance(other, SE3):
            ot, oq = other.data[..., :3], other.data[..., 3:]
            q, oq = torch.broadcast_tensors(q, oq)
            return SE3(torch.cat([_rot(q, ot) + t, _qmul(q, oq)], -1))
        assert other.shape[-1] == 4, other.shape      # homogeneous point (X Y Z W) -> (R XYZ + W t, W)
        W = other[..., 3:]
        return torch.cat([_rot(q, other[..., :3]) + t * W, W], -1)

    def act(self, points):
        return self * points

    def adjT(self, a):
        """a . Ad(X) on the last axis: with Ad = [[R, [t]x R], [0, R]] the row (a_tau, a_phi) becomes
        (R^T a_tau, R^T (a_tau x t + a_phi))."""
        t, q = self.data[..., :3], self.data[..., 3:]
        qi = q * q.new_tensor([-1.0, -1.0, -1.0, 1.0])
        at, ap = a[..., :3], a[..., 3:]
        at_b, t_b = torch.broadcast_tensors(at, t)
        return torch.cat([_rot(qi, at), _rot(qi, torch.linalg.cross(at_b, t_b) + ap)], -1)

    def retr(self, dx):
        """exp(dx) . X"""
        return SE3.exp(dx) * self

    def matrix(self):
        eye = torch.eye(4, dtype=self.data.dtype)
        cols = [self * eye[k].expand(*self.shape, 4) for k in range(4)]
        return torch.stack(cols, -1)


class Sim3:
    """a name for `isinstance` tests; no program run here builds one"""
    manifold_dim = 7


class SO3:
    manifold_dim = 3
