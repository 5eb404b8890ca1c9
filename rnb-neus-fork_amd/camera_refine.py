"""Per-view camera corrections on top of a capture's stored cameras: what `DeviceRays.set_refinement` samples through.

A capture calibrated by structure from motion has noisy poses and focal lengths.  `CameraRefinement` holds, per view,
a rotation vector w and a translation tau (`pose_delta` [V,6]) and optionally the log of a focal scale s
(`focal_log_scale` [V]), all zero at the start, and composes them with a stored camera:

    R' = Exp(w) R          t' = t + tau          K'^-1 = diag(e^-s, e^-s, 1) K^-1

(K' = K diag(e^s, e^s, 1): fx, fy and the skew are scaled, the principal point is kept.)  The composition is a handful
of torch ops on 3-vectors, differentiable by torch; the step from the composed camera to the rays, near / far and
per-ray lights is the ray kernel, whose adjoint is `rnb_gen_rays_camera_bwd` (include/rnbneus.h).  At w = tau = 0 and
s = 0 the composed camera equals the stored one bit for bit: Exp(0) is exactly the identity, and every product and sum
above then has exact operands (1 x, 0 x, x + 0).

The parameters are ordinary `nn.Parameter`s for an optimizer of the caller's; `FlatAdam` and the checkpoint layout do
not know them.  Their gradients are those of the rays of the step: under data parallelism they are shard-local like the
other input gradients (sum them over the ranks with a collective of the caller's)."""
from __future__ import annotations

import torch

# Below this |w|^2 Exp's coefficients come from their Taylor series (three terms; the next one is below
# theta^6 / 5040 = 3.1e-12 at theta = 0.05, under one float64 ulp of the second term's rounding and far under a float32
# ulp).  The closed forms are 0/0 in value and gradient at w = 0, where every refinement starts, and float32
# (1 - cos theta) / theta^2 has lost its digits by the 1e-3 rad a refinement moves by.
SERIES_THETA = 0.05


def _mm3(a, b):
    """a @ b for [...,3,3] operands as a broadcast product and a 3-term sum: exact where one factor is the identity."""
    return (a.unsqueeze(-1) * b.unsqueeze(-3)).sum(-2)


def so3_exp(w):
    """Rodrigues: Exp(w) = I + A [w]x + B [w]x^2 for rotation vectors w [...,3], with A = sin(theta) / theta and
    B = 2 sin^2(theta / 2) / theta^2 (no cancellation), both from their series below `SERIES_THETA`."""
    t2 = (w * w).sum(-1)
    small = t2 < SERIES_THETA * SERIES_THETA
    t2s = torch.where(small, torch.ones_like(t2), t2)       # the closed forms never see the small angles
    th = t2s.sqrt()
    A = torch.where(small, 1.0 - t2 / 6.0 + t2 * t2 / 120.0, th.sin() / th)
    B = torch.where(small, 0.5 - t2 / 24.0 + t2 * t2 / 720.0, 2.0 * (0.5 * th).sin() ** 2 / t2s)
    x, y, z = w.unbind(-1)
    o = torch.zeros_like(x)
    K = torch.stack([o, -z, y, z, o, -x, -y, x, o], dim=-1).reshape(w.shape[:-1] + (3, 3))
    eye = torch.eye(3, dtype=w.dtype, device=w.device)
    return eye + A[..., None, None] * K + B[..., None, None] * _mm3(K, K)


def compose_pose(pose, w, tau):
    """[...,4,4] poses with R' = Exp(w) R and t' = t + tau (the last row is the stored one)."""
    top = torch.cat([_mm3(so3_exp(w), pose[..., :3, :3]), (pose[..., :3, 3] + tau).unsqueeze(-1)], dim=-1)
    return torch.cat([top, pose[..., 3:, :]], dim=-2)


def scale_intrinsics_inv(intrinsics_inv, s):
    """[...,4,4] inverse intrinsics with rows 0 and 1 scaled by e^-s (s [...])."""
    e = torch.exp(-s)
    one = torch.ones_like(e)
    return intrinsics_inv * torch.stack([e, e, one, one], dim=-1).unsqueeze(-1)


class CameraRefinement(torch.nn.Module):
    def __init__(self, n_views, refine_focal=False):
        super().__init__()
        self.n_views = int(n_views)
        if self.n_views < 1:
            raise ValueError(f"CameraRefinement: n_views {n_views} < 1")
        self.pose_delta = torch.nn.Parameter(torch.zeros(self.n_views, 6))      # (w, tau) per view
        self.focal_log_scale = torch.nn.Parameter(torch.zeros(self.n_views)) if refine_focal else None

    def _view(self, v):
        v = int(v)
        if not 0 <= v < self.n_views:
            raise IndexError(f"view {v} out of range (n_views {self.n_views})")
        return v

    def rotation(self, v):
        """Exp(w_v) [3,3]: what rotates a view's world-space lights along with its camera."""
        return so3_exp(self.pose_delta[self._view(v), :3])

    def camera(self, v, pose, intrinsics_inv):
        """(pose', intrinsics_inv') [4,4] of view `v` from its stored `pose` and `intrinsics_inv`."""
        v = self._view(v)
        d = self.pose_delta[v]
        pose = compose_pose(pose, d[:3], d[3:])
        if self.focal_log_scale is not None:
            intrinsics_inv = scale_intrinsics_inv(intrinsics_inv, self.focal_log_scale[v])
        return pose, intrinsics_inv

    def poses(self, pose_all):
        """The refined poses of all views [V,4,4] from the stored `pose_all` (for writing them out)."""
        self._check_stack(pose_all, "pose_all")
        return compose_pose(pose_all, self.pose_delta[:, :3], self.pose_delta[:, 3:])

    def intrinsics_inv(self, intrinsics_all_inv):
        """The refined inverse intrinsics of all views [V,4,4] from the stored `intrinsics_all_inv`."""
        self._check_stack(intrinsics_all_inv, "intrinsics_all_inv")
        if self.focal_log_scale is None:
            return intrinsics_all_inv
        return scale_intrinsics_inv(intrinsics_all_inv, self.focal_log_scale)

    def _check_stack(self, t, name):
        if tuple(t.shape) != (self.n_views, 4, 4):
            raise ValueError(f"{name} {tuple(t.shape)} is not [{self.n_views}, 4, 4]")
