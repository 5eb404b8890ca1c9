"""Golden vectors of the reference's whole-view ray generation: tests/golden/image_rays_small.npz.

TEST INFRASTRUCTURE ONLY, run on the CPU where the reference checkout is available (RNB_REFERENCE, as
oracle/gen_golden.py).  Drives the reference's own `Dataset.gen_rays_at` (models/dataset.py:300-326),
`near_far_from_sphere` (:448-458) and `gen_rays_between` (:401-446) on a synthetic capture and records plain arrays; the
Dataset is instantiated without its file-reading __init__, `cv2` is an inert placeholder and `.cuda()` the identity
while its methods run (oracle/gen_golden.py::raygen_case does the same).  No reference source is stored.

The capture: V = 3 look-at cameras on the sphere of radius 3 (every central ray passes through the origin, so all
three views see the unit sphere), L = 3 lights, H = 11, W = 16, focal length 20, principal point at the image centre.
Recorded: the dataset tensors; gen_rays_at(v, l) for (v, l) = (0, 1), (1, 2), (2, 3) with near / far and the gathers
at `pixels.round().long()` (exp_runner.py:409-410, :448) — level 2 has ty = 0, 2.5, 5, 7.5, 10, the round-half-to-even
rows; gen_rays_between(0, 2, r, 2) for r = 0, 0.3, 1 together with the interpolated pose the reference built (the
value its last `np.linalg.inv` returned).

    python tools/gen_image_golden.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "image_rays_small.npz")
V, L, H, W, FOCAL, RADIUS = 3, 3, 11, 16, 20.0, 3.0
CAMERA_DIRECTIONS = ((1.0, 0.3, 0.2), (-0.4, 1.0, 0.5), (0.2, -0.6, 1.0))
GEN_AT = ((0, 1), (1, 2), (2, 3))
BETWEEN = (0, 2, (0.0, 0.3, 1.0), 2)


def look_at_pose(direction):
    """Camera-to-world pose (OpenCV axes: x right, y down, z forward) at RADIUS * direction / |direction|, looking at
    the origin."""
    c = torch.tensor(direction, dtype=torch.float64)
    c = RADIUS * c / c.norm()
    z = -c / c.norm()
    up = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    x = torch.linalg.cross(z, up)
    x = x / x.norm()
    y = torch.linalg.cross(z, x)
    pose = torch.eye(4, dtype=torch.float64)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, y, z, c
    return pose.float()


def make_dataset():
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")
    import_reference()
    from models.dataset import Dataset  # type: ignore
    g = torch.Generator().manual_seed(321)
    ds = Dataset.__new__(Dataset)
    ds.H, ds.W, ds.n_images, ds.n_lights = H, W, V, L
    ds.images = torch.rand(V, L, H, W, 3, generator=g)
    ds.images_warmup = torch.rand(V, L, H, W, 3, generator=g)
    ds.masks = (torch.rand(V, H, W, generator=g) > 0.4).float().unsqueeze(3)
    ld = torch.randn(V, L, H, W, 3, generator=g)
    ds.light_directions = ld / ld.norm(dim=-1, keepdim=True)
    lw = torch.randn(V, L, 3, generator=g)
    ds.light_directions_warmup = lw / lw.norm(dim=-1, keepdim=True)
    K = torch.eye(4).repeat(V, 1, 1)
    K[:, 0, 0] = FOCAL
    K[:, 1, 1] = FOCAL
    K[:, 0, 2] = (W - 1) / 2.0
    K[:, 1, 2] = (H - 1) / 2.0
    ds.intrinsics_all_inv = torch.inverse(K)
    ds.pose_all = torch.stack([look_at_pose(d) for d in CAMERA_DIRECTIONS])
    return ds


def main():
    ds = make_dataset()
    out = {"images": ds.images, "images_warmup": ds.images_warmup, "masks": ds.masks,
           "light_directions": ds.light_directions, "light_directions_warmup": ds.light_directions_warmup,
           "intrinsics_all_inv": ds.intrinsics_all_inv, "pose_all": ds.pose_all}
    orig_cuda, orig_inv = torch.Tensor.cuda, np.linalg.inv
    torch.Tensor.cuda = lambda self, *a, **k: self
    inverses = []

    def recording_inv(a):
        r = orig_inv(a)
        inverses.append(np.array(r, copy=True))
        return r

    try:
        for i, (v, l) in enumerate(GEN_AT):
            rays_o, rays_d, px, py = ds.gen_rays_at(v, resolution_level=l)
            Hl, Wl, _ = rays_o.shape
            near, far = ds.near_far_from_sphere(rays_o.reshape(-1, 3), rays_d.reshape(-1, 3))
            ix, iy = px.round().long(), py.round().long()          # exp_runner.py:409-410
            pre = f"at{i}_"
            out.update({pre + "img_idx": torch.tensor(v), pre + "level": torch.tensor(l),
                        pre + "rays_o": rays_o.contiguous(), pre + "rays_d": rays_d.contiguous(),
                        pre + "pixels_x": px.contiguous(), pre + "pixels_y": py.contiguous(),
                        pre + "near": near.reshape(Hl, Wl), pre + "far": far.reshape(Hl, Wl),
                        # exp_runner.py:448 for every light idl: light_directions[v, idl, py, px, :]
                        pre + "lights_dir": torch.stack([ds.light_directions[v, idl, iy, ix, :] for idl in range(L)]),
                        pre + "images": torch.stack([ds.images[v, idl, iy, ix, :] for idl in range(L)]),
                        pre + "images_warmup": torch.stack([ds.images_warmup[v, idl, iy, ix, :] for idl in range(L)]),
                        pre + "mask": ds.masks[v, iy, ix, 0]})
        i0, i1, ratios, level = BETWEEN
        np.linalg.inv = recording_inv
        for i, r in enumerate(ratios):
            del inverses[:]
            rays_o, rays_d = ds.gen_rays_between(i0, i1, r, resolution_level=level)
            assert len(inverses) == 3                              # pose_0^-1, pose_1^-1, the interpolated pose
            pre = f"bt{i}_"
            out.update({pre + "idx": torch.tensor([i0, i1]), pre + "ratio": torch.tensor(r, dtype=torch.float64),
                        pre + "level": torch.tensor(level), pre + "rays_o": rays_o.contiguous(),
                        pre + "rays_d": rays_d.contiguous(), pre + "pose": torch.from_numpy(inverses[2])})
    finally:
        torch.Tensor.cuda = orig_cuda
        np.linalg.inv = orig_inv
    np.savez_compressed(OUT, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KiB")


if __name__ == "__main__":
    main()
