"""Shared by tests/test_camera_refine_host.py and tests/test_gpu_camera_refine.py (not a test): a torch restatement, in
whatever dtype its arguments have, of what the ray kernels make of a camera (csrc/raygen.hip pixel_ray + store_ray and
the source-mode light rotation) and of `CameraRefinement.camera`, so that torch autograd in fp64 / fp32 gives the
reference gradients; plus the fixtures' cameras and pixel draws.

Written from the contract in include/rnbneus.h, not from the package: Exp is Rodrigues with five series terms below
0.1 rad (the next term is 1e-10 / 4e7) and the closed forms above, chosen by a host branch."""
import math

import numpy as np
import torch

from tests import source_maps_util as U
from tests.golden_util import load_raygen

TILT, SLANT, SLANT_WARMUP = (0, 120, 240), 54.74, 30


def so3_exp(w):
    """Exp of a rotation vector [3] -> [3,3]"""
    t2 = (w * w).sum()
    if float(t2.detach()) < 0.01:
        A = 1 - t2 / 6 + t2 ** 2 / 120 - t2 ** 3 / 5040 + t2 ** 4 / 362880
        B = 0.5 - t2 / 24 + t2 ** 2 / 720 - t2 ** 3 / 40320 + t2 ** 4 / 3628800
    else:
        th = t2.sqrt()
        A, B = th.sin() / th, 2 * (th / 2).sin() ** 2 / t2
    o = torch.zeros((), dtype=w.dtype)
    K = torch.stack([torch.stack([o, -w[2], w[1]]), torch.stack([w[2], o, -w[0]]), torch.stack([-w[1], w[0], o])])
    return torch.eye(3, dtype=w.dtype) + A * K + B * (K @ K)


def camera(delta, s, pose, kinv):
    """delta [6] = (w, tau), s scalar or None; pose, kinv [4,4] -> (pose', kinv', Exp(w))"""
    E = so3_exp(delta[:3])
    top = torch.cat([E @ pose[:3, :3], (pose[:3, 3] + delta[3:])[:, None]], dim=1)
    pose2 = torch.cat([top, pose[3:]], dim=0)
    if s is None:
        return pose2, kinv, E
    e = torch.exp(-s)
    return pose2, torch.cat([kinv[:2] * e, kinv[2:]], dim=0), E


def rays(kinv, pose, px, py):
    """pixel_ray + store_ray: (rays_o [B,3], rays_d [B,3], near [B,1], far [B,1]) of the pixels (px, py)"""
    q = torch.stack([px.to(kinv.dtype), py.to(kinv.dtype), torch.ones(px.shape[0], dtype=kinv.dtype)], dim=-1)
    p = q @ kinv[:3, :3].T
    v = p / p.norm(dim=-1, keepdim=True)
    d = v @ pose[:3, :3].T
    o = pose[:3, 3].expand(d.shape)
    a = (d * d).sum(-1, keepdim=True)
    mid = -(o * d).sum(-1, keepdim=True) / a
    return o, d, mid - 1.0, mid + 1.0


def rotate(lights, rot):
    """rot [3,3] on the last axis of lights"""
    return lights @ rot.T


def adjoint_loss(out, adj):
    """sum of <tensor, adjoint> over the pairs present in both (None = omitted)"""
    tot = 0.0
    for k, g in adj.items():
        if g is not None:
            tot = tot + (out[k] * g.to(out[k].dtype)).sum()
    return tot


# ------------------------------------------------------------------------------------------------------------ fixtures
def stack_fixture():
    """tests/golden/raygen_small.npz: the tensors of a 3-view 20 x 24 stack-mode capture"""
    return load_raygen()[0]


def source_fixture():
    """tests/golden/source_maps_small.npz with the camera-space per-pixel lights l_cam [V,L,H,W,3] (float64) of the u8
    maps, from the closed form of tests/source_maps_util.py with the identity as the view's rotation"""
    fx = U.load_fixture()
    local, warm = U.light_table(TILT, SLANT), U.light_table(TILT, SLANT_WARMUP)
    n = U.decode_normals(fx["normals_u8"])
    fx["l_cam"] = np.stack([U.closed_form(n[v], None, np.eye(3), local, warm)[2] for v in range(n.shape[0])])
    fx["warm_cam"] = warm
    return fx


def pixels(B, H, W, seed):
    """B pixels of an H x W image with duplicates (the first is repeated at the end when B > 1, and B may exceed H W)"""
    g = torch.Generator().manual_seed(seed)
    px, py = torch.randint(0, W, (B,), generator=g), torch.randint(0, H, (B,), generator=g)
    if B > 1:
        px[-1], py[-1] = px[0], py[0]
    return px, py


def surface_pixels(kinv, pose, H, W, B, seed, radius=0.45, share=0.75):
    """B pixels of which `share` look at the sphere of `radius` about the origin (where the test networks' surface is),
    drawn with repetition, the rest anywhere: (px, py) int64"""
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    o, d, near, _ = rays(kinv.double(), pose.double(), xs.reshape(-1), ys.reshape(-1))
    closest = (o + (near + 1.0) * d).norm(dim=-1)
    hit = torch.nonzero(closest < radius).reshape(-1)
    assert hit.numel() >= 4, "the view does not look at the sphere"
    g = torch.Generator().manual_seed(seed)
    n_hit = int(math.ceil(share * B))
    pick = torch.cat([hit[torch.randint(0, hit.numel(), (n_hit,), generator=g)],
                      torch.randint(0, H * W, (B - n_hit,), generator=g)])
    return (pick % W).contiguous(), (pick // W).contiguous()
