"""Source mode on the device: `DeviceRays.from_source_maps` (rnb_gen_rays_at_view_from_maps, rnb_gen_rays_grid_from_maps)
built from the fixture's raw maps beside a stack-mode `DeviceRays` built from the reference's finished tensors of the same
capture (tests/golden/source_maps_small.npz, tools/gen_source_maps_golden.py).

Rays, near / far, mask and pixel indices are bit-equal between the modes (one device function); colours are within 2e-6
of the reference's; warm-up lights are bit-equal; main lights pass the light-equivalence check of
tests/source_maps_util.py to 2e-6 (fewer than 25 fp32 roundings on values <= 1: 25 x 2^-24 = 1.5e-6).  Each test prints
the largest difference it saw."""
import numpy as np
import pytest
import torch

from tests import source_maps_util as U
from tests.golden_util import Golden
from tests.gpu_support import R  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, W = 13, 11
RAY_KEYS = ("rays_o", "rays_d", "near", "far", "mask", "pixels_x", "pixels_y")


@pytest.fixture(scope="module")
def fx():
    return U.load_fixture()


def _t(a):
    return torch.from_numpy(a)


@pytest.fixture(scope="module")
def pairs(R, fx):
    """name -> (stack mode, source mode, decoded normals [V,H,W,3] float64, rotations [V,3,3] float64)"""
    kinv, pose = _t(fx["intrinsics_inv"]), _t(fx["pose"])
    rot = fx["pose"][:, :3, :3].astype(np.float64)

    def pair(images, warm, lights, sel, normals, albedo):
        stack = R.DeviceRays(_t(images), _t(warm), _t(fx["masks"][sel]), _t(lights), _t(fx["light_directions_warmup"][sel]),
                             kinv[sel], pose[sel], DEV)
        source = R.DeviceRays.from_source_maps(normals, albedo, fx["masks_u8"][sel], kinv[sel], pose[sel], DEV)
        return stack, source, U.decode_normals(np.asarray(normals)), rot[sel]

    return {"u8": pair(fx["images"], fx["images_warmup"], fx["light_directions"], slice(0, 3), fx["normals_u8"], fx["albedo_u8"]),
            "u16": pair(fx["u16_images"][None], fx["u16_images_warmup"][None], fx["u16_light_directions"][None], slice(1, 2),
                        fx["normals_u16"][None], _t(fx["albedo_u16"][None])),
            "no_albedo": pair(fx["noalbedo_images"][None], fx["noalbedo_images_warmup"][None], fx["light_directions"][:1],
                              slice(0, 1), _t(fx["normals_u8"][:1]), None)}


def _pixels(B, seed):
    g = torch.Generator().manual_seed(seed)
    px, py = torch.randint(0, W, (B,), generator=g), torch.randint(0, H, (B,), generator=g)
    if B >= 8:
        px[:4], py[:4] = torch.tensor([0, W - 1, 0, W - 1]), torch.tensor([0, 0, H - 1, H - 1])     # the corners
        px[4:8], py[4:8] = px[:4], py[:4]                                                          # and duplicates
    return px, py


def _close(got, ref, what, seen):
    d = float((got.double().cpu() - ref.double().cpu()).abs().max())
    seen[what] = max(seen.get(what, 0.0), d)
    assert d <= U.RGB_BOUND, f"{what}: {d:.3e} > {U.RGB_BOUND:.1e}"


def _lights_equivalent(got, ref, axis, what, seen):
    """got, ref [L,n,3] tensors, axis [n,3] float64 world axes"""
    d = float(U.light_equivalence_error(ref.cpu().numpy(), got.cpu().numpy(), axis).max())
    seen[what] = max(seen.get(what, 0.0), d)
    assert d <= U.LIGHT_BOUND, f"{what}: {d:.3e} > {U.LIGHT_BOUND:.1e}"


def test_modes_and_resident_bytes(R, pairs):
    stack, source, _, _ = pairs["u8"]
    assert source.source_mode and not stack.source_mode
    assert source.images is None and source.images_warmup is None and source.light_directions is None
    assert source.n_lights == 3 and (source.n_images, source.H, source.W) == (3, H, W)
    assert source.normals.dtype == torch.uint8 and source.masks.shape == (3, H, W, 1)
    assert pairs["u16"][1].normals.dtype == torch.uint16 and pairs["no_albedo"][1].albedos is None
    small = 3 * (16 + 16 + 9) * 4                       # intrinsics, poses and warm-up lights
    assert stack.resident_bytes() == 3 * H * W * 112 + small      # 27 floats and a mask float per pixel
    assert source.resident_bytes() == 3 * H * W * 7 + small       # 3 + 3 + 1 bytes per pixel
    with pytest.raises(ValueError, match="materialize"):
        stack.materialize(0)
    with pytest.raises(IndexError):
        source.sample(3, 4)
    with pytest.raises(IndexError):
        source.sample(0, 2, pixels_x=torch.tensor([0, W]), pixels_y=torch.tensor([0, 0]))


@pytest.mark.parametrize("B", [300, 1])
def test_step_sampling(R, fx, pairs, B):
    """B = 300: more than one 256-thread block, no multiple of 64, the four corners and duplicates"""
    seen = {}
    for name, (stack, source, normals, rot) in pairs.items():
        for v in range(source.n_images):
            px, py = _pixels(B, 11 + v)
            axis = U.world_axis(normals[v][py.numpy(), px.numpy()], rot[v])
            a, b = stack.sample(v, B, pixels_x=px, pixels_y=py), source.sample(v, B, pixels_x=px, pixels_y=py)
            for k in RAY_KEYS:
                assert torch.equal(a[k], b[k]), (name, v, k)
            assert b["true_rgb"].shape == (3, B, 3) and b["lights_dir"].shape == (3, B, 1, 3)
            _close(b["true_rgb"], a["true_rgb"], "true_rgb", seen)
            _lights_equivalent(b["lights_dir"].reshape(3, B, 3), a["lights_dir"].reshape(3, B, 3), axis, "lights_dir", seen)
            assert torch.equal(source.light_directions_at(v, py, px), b["lights_dir"].reshape(3, B, 3))
            a, b = (m.sample(v, B, warmup=True, pixels_x=px, pixels_y=py) for m in (stack, source))
            for k in RAY_KEYS:
                assert torch.equal(a[k], b[k]), (name, v, k, "warmup")
            assert b["lights_dir"].shape == (3, 1, 1, 3) and torch.equal(a["lights_dir"], b["lights_dir"])
            _close(b["true_rgb"], a["true_rgb"], "true_rgb_warmup", seen)
            a, b = (m.ps_gen_random_rays_at_view_on_all_lights(v, B, px, py) for m in (stack, source))
            assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
            assert b[1].shape == (3, B, 3) and b[2].shape == (3, B, 3)
            _close(b[1], a[1], "true_rgb_warmup", seen)
            _close(b[2], a[2], "true_rgb", seen)
    # the stack-mode gathers are the fixture's own values (tests/test_gpu_raygen.py holds them bit-equal)
    stack = pairs["u8"][0]
    px, py = _pixels(B, 11)
    assert torch.equal(stack.sample(0, B, pixels_x=px, pixels_y=py)["true_rgb"].cpu(), _t(fx["images"][0])[:, py, px])
    print(f"SOURCE step sampling B {B}: largest differences {seen}")


def test_whole_views_materialize(R, fx, pairs):
    seen = {}
    ref = {"u8": (fx["images"], fx["images_warmup"], fx["light_directions"], fx["masks"]),
           "u16": (fx["u16_images"][None], fx["u16_images_warmup"][None], fx["u16_light_directions"][None], fx["masks"][1:2]),
           "no_albedo": (fx["noalbedo_images"][None], fx["noalbedo_images_warmup"][None], fx["light_directions"][:1], fx["masks"][:1])}
    for name, (stack, source, normals, rot) in pairs.items():
        for v in range(source.n_images):
            m = source.materialize(v)
            images, warm, lights, masks = (r[v] for r in ref[name])
            assert m["images"].shape == (3, H, W, 3) and m["images_warmup"].shape == (3, H, W, 3)
            assert m["light_directions"].shape == (3, H, W, 3) and m["mask"].shape == (H, W, 1)
            _close(m["images"], _t(images), f"{name} images", seen)
            _close(m["images_warmup"], _t(warm), f"{name} images_warmup", seen)
            assert torch.equal(m["mask"].cpu(), _t(masks))
            _lights_equivalent(m["light_directions"].reshape(3, H * W, 3), _t(lights).reshape(3, H * W, 3),
                               U.world_axis(normals[v].reshape(H * W, 3), rot[v]), f"{name} light_directions", seen)
            full_a, full_b = stack.view_rays(v), source.view_rays(v)
            for k in RAY_KEYS:
                assert torch.equal(full_a[k], full_b[k]), (name, v, k)
    print(f"SOURCE whole views: largest differences {seen}")


def test_view_ranges_and_other_poses(R, pairs):
    """a range of a half-resolution grid with one light (rows 2.4, 4.8, ... and the half-way columns 2.5 and 7.5), and an
    interpolated pose with the view's own gathers: rays bit-equal to stack mode, gathers bit-equal to source mode's
    step kernel at the rounded pixels"""
    stack, source, _, _ = pairs["u8"]
    for v in range(3):
        for kw in (dict(light=1, first=7, count=20), dict(pose=source.pose_between(0, 2, 0.3)),
                   dict(pose=source.pose_between(0, 2, 0.3), light=2, first=3, count=9)):
            a, b = stack.view_rays(v, resolution_level=2, **kw), source.view_rays(v, resolution_level=2, **kw)
            for k in RAY_KEYS:
                assert torch.equal(a[k], b[k]), (v, kw, k)
            n = b["rays_o"].shape[0]
            px, py = b["pixels_x"].round().long(), b["pixels_y"].round().long()
            s = source.sample(v, n, pixels_x=px, pixels_y=py)
            sel = slice(None) if "light" not in kw else slice(kw["light"], kw["light"] + 1)
            assert b["true_rgb"].shape == s["true_rgb"][sel].shape and b["lights_dir"].shape == s["lights_dir"][sel].shape
            assert torch.equal(b["true_rgb"], s["true_rgb"][sel]) and torch.equal(b["lights_dir"], s["lights_dir"][sel])
            assert torch.equal(b["mask"], s["mask"])
            wa, wb = (m.view_rays(v, resolution_level=2, warmup=True, **kw) for m in (stack, source))
            sw = source.sample(v, n, warmup=True, pixels_x=px, pixels_y=py)
            assert torch.equal(wb["true_rgb"], sw["true_rgb"][sel]) and torch.equal(wa["lights_dir"], wb["lights_dir"])
    assert [float(x) for x in source.view_rays(0, resolution_level=2)["pixels_x"][:5]] == [0.0, 2.5, 5.0, 7.5, 10.0]
    # pose-only views need no maps: the stack-mode kernel, no gathers
    a, b = stack.view_rays(pose=source.pose_between(0, 2, 0.3)), source.view_rays(pose=source.pose_between(0, 2, 0.3))
    assert b["mask"] is None and b["true_rgb"] is None and b["lights_dir"] is None
    assert torch.equal(a["rays_d"], b["rays_d"]) and torch.equal(a["near"], b["near"])
    ra, rb = stack.gen_rays_at(1, 2), source.gen_rays_at(1, 2)
    assert all(torch.equal(x, y) for x, y in zip(ra, rb))
    ra, rb = stack.gen_rays_between(0, 1, 0.4, 2), source.gen_rays_between(0, 1, 0.4, 2)
    assert all(torch.equal(x, y) for x, y in zip(ra, rb))
    with pytest.raises(IndexError):
        source.view_rays(1, light=3)
    with pytest.raises(IndexError):
        source.view_rays(1, first=H * W - 3, count=4)


def test_float_maps(R, fx, pairs):
    """already decoded float32 maps give the uint8 results bit for bit; a zero normal gives zero colours and the lights of
    the frame a = (0, 0, 1); a NaN normal gives NaN at its pixel only"""
    _, source, _, rot = pairs["u8"]
    c = _t(fx["normals_u8"]).float() / 255.0
    normals = (c * 2.0 - 1.0) * torch.tensor([1.0, -1.0, -1.0])
    albedo, masks = _t(fx["albedo_u8"]).float() / 255.0, _t(fx["masks_u8"]).float() / 255.0
    kinv, pose = _t(fx["intrinsics_inv"]), _t(fx["pose"])
    fl = R.DeviceRays.from_source_maps(normals, albedo, masks, kinv, pose, DEV)
    assert fl.normals.dtype == torch.float32 and fl.resident_bytes() > 4 * source.resident_bytes() - 2000
    want = [source.materialize(v) for v in range(3)]
    for v in range(3):
        got = fl.materialize(v)
        for k in want[v]:
            assert torch.equal(got[k], want[v][k]), (v, k)
    zero_at, nan_at = (2, 3), (5, 6)
    broken = normals.clone()
    broken[1, zero_at[0], zero_at[1]] = 0.0
    broken[1, nan_at[0], nan_at[1], 1] = float("nan")
    br = R.DeviceRays.from_source_maps(broken, albedo, masks, kinv, pose, DEV)
    got = br.materialize(1)
    torch.cuda.synchronize()
    same = torch.ones(H, W, dtype=torch.bool)
    same[zero_at], same[nan_at] = False, False
    for k in ("images", "images_warmup", "light_directions"):
        g, w = got[k].cpu(), want[1][k].cpu()
        assert torch.equal(g[:, same], w[:, same]), k
        assert bool(torch.isnan(g[:, nan_at[0], nan_at[1]]).all()), k
    assert torch.equal(got["mask"], want[1]["mask"])
    assert bool((got["images"][:, zero_at[0], zero_at[1]] == 0).all())
    assert bool((got["images_warmup"][:, zero_at[0], zero_at[1]] == 0).all())
    lz = got["light_directions"][:, zero_at[0], zero_at[1]].double().cpu().numpy()            # [L,3]
    assert np.isfinite(lz).all()
    local = R.raygen.light_tables()[0]
    assert float(np.abs(lz - local @ rot[1].T).max()) <= U.LIGHT_BOUND          # b1 = x, b2 = y, a = z, rotated to world
    gram = lz @ lz.T
    assert float(np.abs(np.diag(gram) - 1.0).max()) <= 2 * U.LIGHT_BOUND
    # the three lights are orthogonal up to the table's 54.74 degrees for acos(1/sqrt 3): 1 - 1.5 sin^2 = -8e-5
    assert float(np.abs(gram - np.diag(np.diag(gram))).max()) <= 2e-4
    s = br.sample(1, 2, pixels_x=torch.tensor([zero_at[1], nan_at[1]]), pixels_y=torch.tensor([zero_at[0], nan_at[0]]))
    torch.cuda.synchronize()
    assert bool(torch.isnan(s["true_rgb"][:, 1]).all()) and bool((s["true_rgb"][:, 0] == 0).all())
    assert bool(torch.isfinite(s["rays_d"]).all()) and bool(torch.isfinite(s["near"]).all())


def test_through_the_renderer(R, pairs):
    """the warm-up render of a whole view: the rays and the (shared) warm-up lights are identical between the modes, so
    every rendered map is; the gathered mask too, and the gathered warm-up colours to the colour bound.  The main-phase
    render runs on source-mode lights and gives finite maps of the right shapes."""
    stack, source, _, _ = pairs["u8"]
    g = Golden("tiny_main_sharp")
    sdf, dev, col, ren = R.build_from_named_params(g.mc, g.params(), DEV)
    kw = dict(img_idx=0, warmup=True, resolution_level=1, perturb_overwrite=0, cos_anneal_ratio=1.0)
    a, b = ren.render_image(stack, **kw), ren.render_image(source, **kw)
    assert set(a) == set(b) and {"color", "normal", "depth", "weight_sum"} <= set(b)
    seen = {}
    for k in a:
        if k == "true_rgb":
            _close(b[k], a[k], "render_image true_rgb (warm-up)", seen)
        else:
            assert torch.equal(a[k], b[k]), k
    assert b["color"].shape == (3, H, W, 3)
    m = ren.render_image(source, img_idx=0, resolution_level=1, perturb_overwrite=0, cos_anneal_ratio=1.0)
    assert m["color"].shape == (3, H, W, 3) and m["normal"].shape == (H, W, 3) and m["depth"].shape == (H, W)
    assert m["weight_sum"].shape == (H, W) and m["mask"].shape == (H, W) and m["true_rgb"].shape == (3, H, W, 3)
    assert all(bool(torch.isfinite(v).all()) for v in m.values())
    one = ren.render_image(source, img_idx=2, light=1, resolution_level=2, perturb_overwrite=0, chunk_rays=16)
    assert one["color"].shape == (1, 6, 5, 3) and bool(torch.isfinite(one["color"]).all())
    print(f"SOURCE renderer: largest differences {seen}")
