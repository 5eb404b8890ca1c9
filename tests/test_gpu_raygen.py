"""GPU parity of the device-resident ray / target generation (rnb_gen_rays_at_view, DeviceRays) against the
golden vectors of the reference's Dataset methods and against the oracle.  Gathers (colours, mask, lights) are
bit-exact; ray directions / near / far within 1e-6 (a 3-term dot product whose fused / unfused evaluation is
not specified by torch.matmul); against the kernel's own stated arithmetic (tests/raygen_ref.py) they are bit-exact too."""
import os

import numpy as np
import pytest
import torch

from oracle import rnb_oracle as O
from tests import raygen_ref, source_maps_util
from tests.golden_util import GOLDEN_DIR, load_raygen
from tests.gpu_support import R  # noqa: F401

pytestmark = pytest.mark.gpu


def _rays(R, ds):
    return R.DeviceRays(ds["images"], ds["images_warmup"], ds["masks"], ds["light_directions"],
                        ds["light_directions_warmup"], ds["intrinsics_all_inv"], ds["pose_all"], "cuda:0")


def test_reference_method_signature_and_values(R):
    ds, cases = load_raygen()
    dr = _rays(R, ds)
    for c in cases:
        v, B = int(c["img_idx"]), c["pixels_x"].numel()
        data, wu, rgb, px, py = dr.ps_gen_random_rays_at_view_on_all_lights(v, B, c["pixels_x"], c["pixels_y"])
        assert data.shape == (B, 7) and wu.shape == (3, B, 3) and rgb.shape == (3, B, 3)
        assert torch.equal(px.cpu(), c["pixels_x"]) and torch.equal(py.cpu(), c["pixels_y"])
        assert torch.equal(rgb.cpu(), c["images"]) and torch.equal(wu.cpu(), c["images_warmup"])
        assert torch.equal(data[:, 6].cpu(), c["data"][:, 6])                 # mask
        assert torch.equal(data[:, :3].cpu(), c["data"][:, :3])               # rays_o: a copy of the pose
        torch.testing.assert_close(data[:, 3:6].cpu(), c["data"][:, 3:6], rtol=0, atol=1e-6)
        near, far = dr.near_far_from_sphere(data[:, :3], data[:, 3:6])
        torch.testing.assert_close(near.cpu(), c["near"], rtol=0, atol=2e-6)
        torch.testing.assert_close(far.cpu(), c["far"], rtol=0, atol=2e-6)
        lights = dr.light_directions_at(v, py, px)
        assert torch.equal(lights.cpu(), c["lights_dir"])


@pytest.mark.parametrize("warmup", [False, True])
def test_one_launch_step_inputs(R, warmup):
    ds, cases = load_raygen()
    dr = _rays(R, ds)
    c = cases[2]
    v, B = int(c["img_idx"]), c["pixels_x"].numel()
    s = dr.sample(v, B, warmup=warmup, pixels_x=c["pixels_x"], pixels_y=c["pixels_y"])
    ref = O.gen_rays_at_view(ds, v, c["pixels_x"], c["pixels_y"])
    assert s["rays_o"].shape == (B, 3) and s["mask"].shape == (B, 1) and s["near"].shape == (B, 1)
    torch.testing.assert_close(s["rays_d"].cpu(), ref["data"][:, 3:6], rtol=0, atol=1e-6)
    torch.testing.assert_close(s["near"].cpu(), ref["near"], rtol=0, atol=2e-6)
    torch.testing.assert_close(s["far"].cpu(), ref["far"], rtol=0, atol=2e-6)
    if warmup:
        assert torch.equal(s["true_rgb"].cpu(), ref["images_warmup"])
        assert s["lights_dir"].shape == (3, 1, 1, 3)
        assert torch.equal(s["lights_dir"].reshape(3, 3).cpu(), ds["light_directions_warmup"][v])
    else:
        assert torch.equal(s["true_rgb"].cpu(), ref["images"])
        assert s["lights_dir"].shape == (3, B, 1, 3)
        assert torch.equal(s["lights_dir"].reshape(3, B, 3).cpu(), ref["lights_dir"])


def test_device_draws_single_ray_and_bad_indices(R):
    ds, cases = load_raygen()
    dr = _rays(R, ds)
    s = dr.sample(1, 4096)                       # pixels drawn on the device
    px, py = s["pixels_x"].cpu(), s["pixels_y"].cpu()
    assert int(px.min()) >= 0 and int(px.max()) < dr.W and int(py.min()) >= 0 and int(py.max()) < dr.H
    assert len(torch.unique(py * dr.W + px)) > 400          # 480 pixels, 4096 draws: nearly all are hit
    ref = O.gen_rays_at_view(ds, 1, px, py)
    assert torch.equal(s["true_rgb"].cpu(), ref["images"])
    one = dr.sample(0, 1, pixels_x=torch.tensor([3]), pixels_y=torch.tensor([5]))   # B = 1 (the reference's
    assert one["rays_d"].shape == (1, 3)                                              # .squeeze() breaks there)
    assert torch.equal(one["true_rgb"].cpu()[:, 0], ds["images"][0, :, 5, 3])
    with pytest.raises(IndexError):
        dr.sample(7, 4)
    with pytest.raises(IndexError):                                  # host pixel indices are range-checked
        dr.sample(0, 2, pixels_x=torch.tensor([0, dr.W]), pixels_y=torch.tensor([0, 0]))
    with pytest.raises(ValueError):
        dr.sample(0, 4, pixels_x=torch.tensor([1, 2]), pixels_y=torch.tensor([1, 2]))


# ------------------------------------------------------------------------------------- the stated arithmetic, bit for bit
def _ray_builds(R, front, targets):
    """a DeviceRays on the fixture that drives one of the kernel's four instantiations"""
    if targets == "maps":
        fx = source_maps_util.load_fixture()
        return R.DeviceRays.from_source_maps(fx["normals_u8"], fx["albedo_u8"], fx["masks_u8"], torch.from_numpy(
            fx["intrinsics_inv"]), torch.from_numpy(fx["pose"]), "cuda:0")
    if front == "list":
        return _rays(R, load_raygen()[0])
    z = np.load(os.path.join(GOLDEN_DIR, "image_rays_small.npz"), allow_pickle=False)
    return _rays(R, {k: torch.from_numpy(z[k]) for k in z.files})


def _assert_ray_bits(got, kinv, pose, x, y, what):
    want = raygen_ref.pixel_rays(kinv.cpu().numpy(), np.asarray(pose.cpu() if torch.is_tensor(pose) else pose), x.cpu().numpy(),
                                 y.cpu().numpy())
    for k, w in zip(("rays_o", "rays_d", "near", "far"), want):
        assert got[k].dtype == torch.float32 and torch.equal(got[k].cpu(), torch.from_numpy(w)), (what, k)


@pytest.mark.parametrize("targets", ["stack", "maps"])
@pytest.mark.parametrize("front", ["list", "grid"])
def test_ray_bits_follow_the_stated_arithmetic(R, front, targets):
    """rays_o, rays_d, near, far of every instantiation of the ray kernel (pixel list or grid range, stack gathers or
    source maps) are the bits of tests/raygen_ref.py: float32, three-term sums left to right, IEEE sqrt and division, no
    fused multiply-add.  List: B = 1, and B = 257 (a second 256-thread workgroup with one live lane).  Grid: a whole view
    at level 1; at level 2 a range that starts and ends inside a row, with one light and with all; a pose-only call."""
    dr = _ray_builds(R, front, targets)
    if front == "list":
        for v, B in ((0, 1), (2, 257)):
            g = torch.Generator().manual_seed(5 + B)
            px, py = torch.randint(0, dr.W, (B,), generator=g), torch.randint(0, dr.H, (B,), generator=g)
            for warmup in (False, True):
                s = dr.sample(v, B, warmup=warmup, pixels_x=px, pixels_y=py)
                assert s["rays_d"].shape == (B, 3) and s["near"].shape == (B, 1)
                _assert_ray_bits(s, dr.intrinsics_all_inv[v], dr.pose_all[v], px, py, (front, targets, B, warmup))
        return
    Wl = dr.W // 2
    first, count = Wl + 2, 2 * Wl + 1          # starts at column 2 of row 1, ends after column 2 of row 3
    assert first % Wl and (first + count) % Wl and first + count < (dr.H // 2) * Wl
    calls = [(1, dict(resolution_level=1)), (0, dict(resolution_level=2, first=first, count=count, light=1)),
             (2, dict(resolution_level=2, first=first, count=count))]
    for v, kw in calls:
        r = dr.view_rays(v, **kw)
        assert r["rays_d"].shape[0] == kw.get("count", dr.H * dr.W) and r["true_rgb"].shape[0] == (1 if "light" in kw else 3)
        _assert_ray_bits(r, dr.intrinsics_all_inv[v], dr.pose_all[v], r["pixels_x"], r["pixels_y"], (front, targets, kw))
    pose = dr.pose_between(0, 2, 0.3)                                   # pose only: no mask, no targets (view 0's intrinsics)
    r = dr.view_rays(pose=pose, resolution_level=2)
    assert r["mask"] is None and r["true_rgb"] is None and r["rays_d"].shape[0] == (dr.H // 2) * Wl
    _assert_ray_bits(r, dr.intrinsics_all_inv[0], pose, r["pixels_x"], r["pixels_y"], (front, targets, "pose only"))
