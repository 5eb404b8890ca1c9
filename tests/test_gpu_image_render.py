"""Whole views on the device: rnb_gen_rays_grid / DeviceRays.gen_rays_at, gen_rays_between, view_rays against the reference's
own rays (tests/golden/image_rays_small.npz, tools/gen_image_golden.py), and NeuSRenderer.render_image against the CPU
oracle on the device's depths by the calibrated output rule of tests/parity.py."""
import os

import numpy as np
import pytest
import torch

from oracle import rnb_oracle as O
from tests import parity as P
from tests.golden_util import POSE_BOUND, Golden
from tests.gpu_support import R  # noqa: F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_rays_small.npz")
DS_KEYS = ("images", "images_warmup", "masks", "light_directions", "light_directions_warmup", "intrinsics_all_inv", "pose_all")


@pytest.fixture(scope="module")
def fx():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _rays(R, fx):
    return R.DeviceRays(*[fx[k] for k in DS_KEYS], "cuda:0")


# ------------------------------------------------------------------------------------------------------------------- 6
def test_gen_rays_at_is_the_references(R, fx):
    """rays_o: a copy of the pose; rays_d / near / far: the bounds tests/test_gpu_raygen.py holds the same arithmetic to;
    pixel coordinates and every gather bit-equal, the half-way rows (2.5 -> 2, 7.5 -> 8) included."""
    dr = _rays(R, fx)
    for i in range(3):
        v, l = int(fx[f"at{i}_img_idx"]), int(fx[f"at{i}_level"])
        pre = f"at{i}_"
        rays_o, rays_d, px, py = dr.gen_rays_at(v, resolution_level=l)
        Hl, Wl = dr.H // l, dr.W // l
        assert rays_o.shape == (Hl, Wl, 3) and rays_d.shape == (Hl, Wl, 3) and px.shape == (Hl, Wl) and py.shape == (Hl, Wl)
        assert torch.equal(rays_o.cpu(), fx[pre + "rays_o"])
        torch.testing.assert_close(rays_d.cpu(), fx[pre + "rays_d"], rtol=0, atol=1e-6)
        assert torch.equal(px.cpu(), fx[pre + "pixels_x"]) and torch.equal(py.cpu(), fx[pre + "pixels_y"])
        r = dr.view_rays(v, resolution_level=l)
        assert r["H"] == Hl and r["W"] == Wl and r["near"].shape == (Hl * Wl, 1)
        torch.testing.assert_close(r["near"].cpu().reshape(Hl, Wl), fx[pre + "near"], rtol=0, atol=2e-6)
        torch.testing.assert_close(r["far"].cpu().reshape(Hl, Wl), fx[pre + "far"], rtol=0, atol=2e-6)
        assert r["lights_dir"].shape == (3, Hl * Wl, 1, 3)
        assert torch.equal(r["lights_dir"].cpu().reshape(3, Hl, Wl, 3), fx[pre + "lights_dir"])
        assert torch.equal(r["true_rgb"].cpu().reshape(3, Hl, Wl, 3), fx[pre + "images"])
        assert torch.equal(r["mask"].cpu().reshape(Hl, Wl), fx[pre + "mask"])
        w = dr.view_rays(v, resolution_level=l, warmup=True, light=2)
        assert torch.equal(w["true_rgb"].cpu().reshape(Hl, Wl, 3), fx[pre + "images_warmup"][2])
        assert w["lights_dir"].shape == (1, 1, 1, 3)
        assert torch.equal(w["lights_dir"].cpu().reshape(3), fx["light_directions_warmup"][v, 2])
        one = dr.view_rays(v, resolution_level=l, light=1)
        assert torch.equal(one["lights_dir"].cpu().reshape(Hl, Wl, 3), fx[pre + "lights_dir"][1])
        assert torch.equal(one["true_rgb"].cpu().reshape(Hl, Wl, 3), fx[pre + "images"][1])
    # the half-to-even rows really differ from half-away-from-zero: rows 2 and 3 of the image are different data
    assert not torch.equal(fx["light_directions"][1, :, 2], fx["light_directions"][1, :, 3])


def test_view_rays_ranges_concatenate_to_the_full_call(R, fx):
    dr = _rays(R, fx)
    full = dr.view_rays(1, resolution_level=1)
    N = dr.H * dr.W
    parts = [dr.view_rays(1, resolution_level=1, first=a, count=b - a) for a, b in ((0, 1), (1, 70), (70, N))]
    for k in ("rays_o", "rays_d", "near", "far", "mask", "pixels_x", "pixels_y"):
        assert torch.equal(torch.cat([p[k] for p in parts], dim=0), full[k]), k
    for k in ("lights_dir", "true_rgb"):
        assert torch.equal(torch.cat([p[k] for p in parts], dim=1), full[k]), k
    with pytest.raises(IndexError):
        dr.view_rays(1, first=N - 3, count=4)
    with pytest.raises(IndexError):
        dr.view_rays(1, light=3)
    with pytest.raises(IndexError):
        dr.view_rays(3)
    with pytest.raises(ValueError):
        dr.view_rays(1, resolution_level=12)


def test_gen_rays_between_is_the_references(R, fx):
    """the bounds of gen_rays_at widened by three times the measured pose difference (tests/golden_util.py POSE_BOUND:
    0.0, so rays_o stays bit-equal)"""
    dr = _rays(R, fx)
    for i in range(3):
        i0, i1 = (int(v) for v in fx[f"bt{i}_idx"])
        rays_o, rays_d = dr.gen_rays_between(i0, i1, float(fx[f"bt{i}_ratio"]), resolution_level=int(fx[f"bt{i}_level"]))
        assert rays_o.shape == fx[f"bt{i}_rays_o"].shape == (5, 8, 3)
        torch.testing.assert_close(rays_o.cpu(), fx[f"bt{i}_rays_o"], rtol=0, atol=3.0 * POSE_BOUND)
        torch.testing.assert_close(rays_d.cpu(), fx[f"bt{i}_rays_d"], rtol=0, atol=1e-6 + 3.0 * POSE_BOUND)
    r = dr.view_rays(pose=dr.pose_between(0, 2, 0.3), resolution_level=2)
    assert r["mask"] is None and r["lights_dir"] is None and r["true_rgb"] is None
    torch.testing.assert_close(r["near"].cpu().reshape(5, 8), O.near_far_from_sphere(
        fx["bt1_rays_o"].reshape(-1, 3), fx["bt1_rays_d"].reshape(-1, 3))[0].reshape(5, 8), rtol=0, atol=2e-6)


# ------------------------------------------------------------------------------------------------------------------- 8
def _rule(got, ref32, ref64, what):
    got = got.reshape(ref64.shape)
    e_hip, e_ref, bound = P.value_errors(got, ref64, ref32)
    print(f"IMAGE {what}: |hip - fp64| {e_hip:.3e}, fp32 oracle {e_ref:.3e}, bound {bound:.3e}")
    P.check_value(what, got, ref64, ref32)


def _oracle_maps(p, mc, rays, lights, z, dt):
    q = {k: v.to(dt) for k, v in p.items()}
    r = O.render_rnb(q, mc, rays["rays_o"].to(dt), rays["rays_d"].to(dt), rays["near"].to(dt), rays["far"].to(dt),
                     lights.to(dt), cos_anneal_ratio=1.0, z_vals=z.to(dt))
    r = {k: v.detach() for k, v in r.items()}
    w = r["weights"]
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 2.0 / mc.render.n_samples)], -1).to(dt)
    mid = z.to(dt) + dists * 0.5
    return {"color": r["color_fine"], "weight_sum": r["weight_sum"],
            "normal": (r["gradients"] * w[:, :, None] * r["inside_sphere"][:, :, None]).sum(dim=1),
            "albedo": (r["sampled_albedo"] * w[:, :, None]).sum(dim=1), "depth": (w * mid).sum(dim=1, keepdim=True)}


@pytest.fixture(scope="module")
def view1(R, fx):
    """view 1 rendered at chunk_rays = 64 (176 rays: two chunks and a partial one) and 176, and the oracle's rays"""
    g = Golden("tiny_main_sharp")
    p = g.params()
    sdf, dev, col, ren = R.build_from_named_params(g.mc, p, "cuda:0")
    dr = _rays(R, fx)
    H, W = dr.H, dr.W
    py, px = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    ds = {k: fx[k] for k in DS_KEYS}
    ref = O.gen_rays_at_view(ds, 1, px.reshape(-1), py.reshape(-1))
    rays = {"rays_o": ref["data"][:, :3], "rays_d": ref["data"][:, 3:6], "near": ref["near"], "far": ref["far"]}
    imgs = {c: ren.render_image(dr, 1, api="render_rnb", perturb_overwrite=0, cos_anneal_ratio=1.0, chunk_rays=c,
                                return_z_vals=True) for c in (64, 176)}
    torch.cuda.synchronize()
    return g, p, ren, dr, rays, ref["lights_dir"].reshape(3, H * W, 1, 3), imgs


@pytest.mark.parametrize("chunk", [64, 176])
def test_render_image_against_the_oracle(R, fx, view1, chunk):
    g, p, ren, dr, rays, lights, imgs = view1
    img = imgs[chunk]
    H, W, N = dr.H, dr.W, dr.H * dr.W
    assert img["color"].shape == (3, H, W, 3) and img["normal"].shape == (H, W, 3) and img["albedo"].shape == (H, W, 3)
    assert img["depth"].shape == (H, W) and img["weight_sum"].shape == (H, W) and img["mask"].shape == (H, W)
    assert img["z_vals"].shape == (N, 32)
    assert torch.equal(img["mask"].cpu(), fx["masks"][1, :, :, 0]) and torch.equal(img["true_rgb"].cpu(), fx["images"][1])
    z = img["z_vals"].cpu()
    assert bool((z[:, 1:] >= z[:, :-1]).all())
    r32 = _oracle_maps(p, g.mc, rays, lights, z, torch.float32)
    r64 = _oracle_maps(p, g.mc, rays, lights, z, torch.float64)
    share = float((r64["weight_sum"] > 0.5).double().mean())
    print(f"IMAGE view 1 chunk {chunk}: share of rays with weight_sum > 0.5 = {share:.2f}")
    assert 0.2 <= share <= 0.8, "degenerate view: (nearly) every ray hits or misses"
    for k in ("color", "normal", "albedo", "depth", "weight_sum"):
        got = img[k].reshape(3, N, 3) if k == "color" else img[k].reshape(N, -1)
        _rule(got, r32[k], r64[k], f"view 1 chunk {chunk} {k}")


def test_chunkings_agree(R, view1):
    """Not bit for bit (the per-64-point-tile fp16 scales make the networks' bits, the sampled depths included, depend on
    where the chunks cut).  Each chunking is within the calibrated bound of the fp64 oracle at its own depths, so the two
    may differ by the sum of the two bounds plus the fp64 oracle's own difference between the two sets of depths."""
    g, p, ren, dr, rays, lights, imgs = view1
    a, b = imgs[64], imgs[176]
    za, zb = a["z_vals"].cpu(), b["z_vals"].cpu()
    print(f"IMAGE chunkings: depths differ by at most {float((za - zb).abs().max()):.3e}")
    ora = {c: (_oracle_maps(p, g.mc, rays, lights, z, torch.float32), _oracle_maps(p, g.mc, rays, lights, z, torch.float64))
           for c, z in ((64, za), (176, zb))}
    for k in ("color", "normal", "albedo", "depth", "weight_sum"):
        bound = float((ora[64][1][k] - ora[176][1][k]).abs().max())
        for c in (64, 176):
            r32, r64 = ora[c]
            bound += P.value_bound(r64[k], P.max_err(r32[k], r64[k]))
        d = float((a[k].double() - b[k].double()).abs().max())
        print(f"IMAGE chunkings {k}: differ by {d:.3e}, bound {bound:.3e}")
        assert d <= bound, f"{k}: the chunkings differ by {d:.3e} > {bound:.3e}"


def test_render_image_other_modes_and_shapes(R, fx, view1):
    g, p, ren, dr, rays, lights, imgs = view1
    img = ren.render_image(dr, 1, api="render_rnb_warmup", light=1, resolution_level=2, perturb_overwrite=0,
                           cos_anneal_ratio=1.0, chunk_rays=16)
    assert img["color"].shape == (1, 5, 8, 3) and img["normal"].shape == (5, 8, 3) and img["weight_sum"].shape == (5, 8)
    assert img["albedo"].shape == (5, 8, 3) and img["depth"].shape == (5, 8)
    assert torch.equal(img["mask"].cpu(), fx["at1_mask"]) and torch.equal(img["true_rgb"].cpu()[0], fx["at1_images"][1])
    assert all(bool(torch.isfinite(v).all()) for v in img.values())
    # the warm-up's shared lights and images, every light
    wu = ren.render_image(dr, 1, warmup=True, resolution_level=2, perturb_overwrite=0, maps=("color", "weight_max"))
    assert wu["color"].shape == (3, 5, 8, 3) and torch.equal(wu["true_rgb"].cpu(), fx["at1_images_warmup"])
    assert set(wu) == {"color", "weight_max", "mask", "true_rgb"}
    # a novel view: render(), no lights, host copies after one synchronisation
    bg = torch.tensor([1.0, 1.0, 1.0])
    nv = ren.render_image(dr, pose=dr.pose_between(0, 2, 0.3), resolution_level=2, perturb_overwrite=0,
                          background_rgb=bg, to_host=True)
    assert set(nv) == {"color", "normal", "depth", "weight_sum", "mask", "true_rgb"} and nv["mask"] is None
    assert isinstance(nv["color"], np.ndarray) and nv["color"].shape == (5, 8, 3) and nv["weight_sum"].shape == (5, 8)
    # the background enters as bg (1 - weight_sum): against the same render without it (same chunks, same depths)
    nb = ren.render_image(dr, pose=dr.pose_between(0, 2, 0.3), resolution_level=2, perturb_overwrite=0, to_host=True)
    assert np.array_equal(nv["weight_sum"], nb["weight_sum"]) and float(nv["weight_sum"].min()) < 0.5
    assert np.allclose(nv["color"] - nb["color"], (1.0 - nv["weight_sum"])[..., None], atol=1e-5)
    with pytest.raises(ValueError, match="lights"):
        ren.render_image(dr, pose=dr.pose_between(0, 2, 0.3), api="render_rnb")
    # under enable_grad: no graph
    with torch.enable_grad():
        out = ren.render_image(dr, 1, resolution_level=2, perturb_overwrite=0, chunk_rays=16)
    assert all(v.grad_fn is None and not v.requires_grad for v in out.values())
