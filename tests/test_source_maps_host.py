"""Host-side checks of source mode (no GPU): the closed form of include/rnbneus.h against what the reference's
`Dataset.gen_light_directions` and dataset preparation gave (tests/golden/source_maps_small.npz,
tools/gen_source_maps_golden.py), the light tables, the camera decomposition, the constructor's refusals and the argument
checks of `rnb_gen_rays_at_view_from_maps` / `rnb_gen_rays_grid_from_maps` that need no device."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import source_maps_util as U

RNB_E_INVALID, RNB_E_NULL = -1, -4
TILT, SLANT, SLANT_WARMUP = (0, 120, 240), 54.74, 30


@pytest.fixture(scope="module")
def R():
    import rnb_neus_fork_amd as pkg
    pkg.native.load()
    return pkg


@pytest.fixture(scope="module")
def fx():
    return U.load_fixture()


def _views(fx):
    """(name, PNG normals, PNG albedo or None, pose index, images, images_warmup, light_directions) of every recorded case"""
    for v in range(3):
        yield f"view {v} u8", fx["normals_u8"][v], fx["albedo_u8"][v], v, fx["images"][v], fx["images_warmup"][v], fx["light_directions"][v]
    yield "view 1 u16", fx["normals_u16"], fx["albedo_u16"], 1, fx["u16_images"], fx["u16_images_warmup"], fx["u16_light_directions"]
    yield "view 0 u8 no_albedo", fx["normals_u8"][0], None, 0, fx["noalbedo_images"], fx["noalbedo_images_warmup"], fx["light_directions"][0]


def test_fixture_holds_the_cases_it_should(fx):
    n = U.decode_normals(fx["normals_u8"])
    assert fx["normals_u8"].shape == (3, 13, 11, 3) and fx["normals_u16"].dtype == np.uint16
    assert int((n[..., 2] > 0).sum()) >= 10                              # back-facing
    assert bool((fx["normals_u8"] == 0).all(axis=-1).any())              # decodes to (-1, 1, 1)
    length = np.linalg.norm(n, axis=-1)
    assert float(length.min()) < 0.6 and float(length.max()) > 1.3       # clearly non-unit
    assert int((np.abs(length - 1.0) < 0.02).sum()) > 300                # unit after quantisation
    assert bool((n[..., 2] != 0).all()) and bool((U.decode_normals(fx["normals_u16"])[..., 2] != 0).all())
    assert set(np.unique(fx["masks_u8"])) >= {0, 127, 128, 255}
    assert not np.array_equal(fx["normals_u16"] >> 8, fx["normals_u8"][1])     # drawn independently


def test_closed_form_is_the_references(fx):
    """The float64 closed form against the fixture over every pixel: images, warm-up images, no_albedo images, masks and
    warm-up lights to 1e-6 (the fixture is rounded to float32), main lights by the light-equivalence check to 2e-6."""
    local, warm = U.light_table(TILT, SLANT), U.light_table(TILT, SLANT_WARMUP)
    worst = {"images": 0.0, "images_warmup": 0.0, "lights": 0.0}
    for name, nv, av, v, images, images_warmup, lights in _views(fx):
        n = U.decode_normals(nv)
        rot = fx["pose"][v, :3, :3].astype(np.float64)
        im, im_w, l_world = U.closed_form(n, None if av is None else U.decode(av), rot, local, warm)
        e_im, e_w = float(np.abs(im - images).max()), float(np.abs(im_w - images_warmup).max())
        e_l = float(U.light_equivalence_error(lights, l_world, U.world_axis(n, rot)).max())
        print(f"SOURCE closed form {name}: images {e_im:.2e}, images_warmup {e_w:.2e}, lights (up to the rotation) {e_l:.2e}")
        assert e_im <= 1e-6 and e_w <= 1e-6 and e_l <= U.LIGHT_BOUND, name
        # the shade is |n| cos(slant) for camera-facing normals, 0 for back-facing ones, whatever the light
        want = np.where(n[..., 2] < 0, np.linalg.norm(n, axis=-1) * np.cos(np.radians(SLANT)), 0.0)
        alb = np.ones_like(n) if av is None else U.decode(av)
        assert float(np.abs(images - (alb * want[..., None])[None]).max()) <= 1e-6, name
        worst = {k: max(worst[k], e) for k, e in zip(("images", "images_warmup", "lights"), (e_im, e_w, e_l))}
    print(f"SOURCE closed form maxima: {worst}")
    masks = (U.decode(fx["masks_u8"]) > 0.5).astype(np.float32)[..., None]
    assert np.array_equal(masks, fx["masks"])
    for v in range(3):
        lw = warm @ fx["pose"][v, :3, :3].astype(np.float64).T
        assert float(np.abs(lw - fx["light_directions_warmup"][v]).max()) <= 1e-6


def test_light_equivalence_check_refuses_wrong_lights(fx):
    """the check is not vacuous: swapped tilts (the other cyclic order), a mirrored frame, a wrong slant and a non-unit
    light all fail it by far"""
    local, warm = U.light_table(TILT, SLANT), U.light_table(TILT, SLANT_WARMUP)
    n = U.decode_normals(fx["normals_u8"][2])
    rot = fx["pose"][2, :3, :3].astype(np.float64)
    axis = U.world_axis(n, rot)
    ref = fx["light_directions"][2]
    _, _, good = U.closed_form(n, None, rot, local, warm)
    assert float(U.light_equivalence_error(ref, good, axis).max()) <= U.LIGHT_BOUND
    assert float(U.light_equivalence_error(ref, good[[0, 2, 1]], axis).min()) > 0.1
    assert float(U.light_equivalence_error(ref, U.closed_form(n, None, rot, U.light_table(TILT, 50.0), warm)[2], axis).min()) > 0.01
    assert float(U.light_equivalence_error(ref, good * 1.001, axis).min()) > 1e-4
    mirrored = good - 2.0 * (good * axis[None]).sum(-1, keepdims=True) * axis[None]
    assert float(U.light_equivalence_error(ref, mirrored, axis).min()) > 0.1


def test_light_tables(R, fx):
    local, warm = R.raygen.light_tables()
    assert local.shape == (3, 3) and local.dtype == np.float64 and warm.dtype == np.float64
    assert float(np.abs(warm - fx["warmup_lights_cam"]).max()) <= 1e-7
    # models/dataset.py:257-266 with the normal given: slant 54.74 degrees
    t, s = np.radians([0, 120, 240]), np.radians([54.74, 54.74, 54.74])
    u = -np.array([np.sin(s) * np.cos(t), np.sin(s) * np.sin(t), np.cos(s)])
    assert float(np.abs(local - u.T).max()) <= 1e-7
    one, _ = R.raygen.light_tables((45,), 20, 10)
    assert one.shape == (1, 3) and abs(float(np.linalg.norm(one)) - 1.0) < 1e-12
    for bad in ((), tuple(range(9))):
        with pytest.raises(ValueError, match="lights"):
            R.raygen.light_tables(bad)


def test_symbols_and_abi(R):
    assert "rnb_gen_rays_at_view_from_maps" in R.native.EXPORTED_SYMBOLS
    assert "rnb_gen_rays_grid_from_maps" in R.native.EXPORTED_SYMBOLS
    assert R.native.load().rnb_abi_version() == 5 and R.native.ABI_VERSION == 5
    # the ctypes mirror has rnb_source_maps_t's layout: three pointers, six int32, two [8][3] float tables
    S = R.native.SourceMaps
    assert C.sizeof(S) == 24 + 24 + 2 * 96 and S.normals_type.offset == 24 and S.n_lights.offset == 44
    assert S.local_lights.offset == 48 and S.warmup_lights_cam.offset == 144


def _source(R, fake, **kw):
    s = R.native.SourceMaps()
    s.normals = s.albedo = s.mask = fake.value
    s.normals_type, s.mask_type, s.H, s.W, s.mask_channels, s.n_lights = R.native.SOURCE_U8, R.native.SOURCE_U8, 13, 11, 1, 3
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_entry_point_argument_checks_need_no_device(R):
    """every refusal comes before the first HIP call: the pointers are host addresses that are never dereferenced"""
    lib = R.native.load()
    host = (C.c_float * 64)()
    fake = C.c_void_p(C.addressof(host))

    def at_view(src="default", B=4, kinv=fake, near=None, far=None, **kw):
        s = _source(R, fake, **kw) if src == "default" else src
        rc = lib.rnb_gen_rays_at_view_from_maps(kinv, fake, None if s is None else C.byref(s), fake, fake, B, fake, None,
                                                None, None, near, far, None)
        return rc, lib.rnb_last_error_string().decode()

    def grid(src="default", first=0, n=40, light=-1, view_pose=fake, Wl=8, Hl=5, near=None, far=None, **kw):
        s = _source(R, fake, **kw) if src == "default" else src
        rc = lib.rnb_gen_rays_grid_from_maps(fake, fake, view_pose, fake, fake, Wl, Hl, first, n,
                                             None if s is None else C.byref(s), light, fake, None, None, None, near, far, None)
        return rc, lib.rnb_last_error_string().decode()

    for call in (at_view, grid):
        for kw in (dict(src=None), dict(normals=None), dict(mask=None), dict(near=fake)):
            rc, msg = call(**kw)
            assert rc == RNB_E_NULL and msg, (call.__name__, kw, rc, msg)
        for kw, word in ((dict(normals_type=3), "type"), (dict(normals_type=-1), "type"), (dict(mask_type=7), "type"),
                         (dict(n_lights=0), "n_lights"), (dict(n_lights=9), "n_lights"), (dict(H=0), "shape"),
                         (dict(mask_channels=0), "shape")):
            rc, msg = call(**kw)
            assert rc == RNB_E_INVALID and word in msg, (call.__name__, kw, rc, msg)
    assert at_view(kinv=None)[0] == RNB_E_NULL
    rc, msg = at_view(B=0)
    assert rc == RNB_E_INVALID and "shape" in msg
    assert grid(view_pose=None)[0] == RNB_E_NULL
    for kw, word in ((dict(first=1, n=40), "outside"), (dict(first=-1, n=4), "outside"), (dict(n=0), "outside"),
                     (dict(light=3), "light"), (dict(light=-2), "light"), (dict(light=1, n_lights=1), "light"),
                     (dict(Wl=0), "shape")):
        rc, msg = grid(**kw)
        assert rc == RNB_E_INVALID and word in msg, (kw, rc, msg)


def test_constructor_refusals_come_before_the_device(R, fx):
    """dtype and shape mismatches and more than 8 lights are ValueErrors raised before anything touches a device (the
    device given here is the CPU, which is refused last)"""
    n, a, m = fx["normals_u8"], fx["albedo_u8"], fx["masks_u8"]
    kinv, pose = fx["intrinsics_inv"], fx["pose"]
    make = R.DeviceRays.from_source_maps
    for args, word in (((n.astype(np.int32), a, m, kinv, pose), "uint8, uint16 or float32"),
                       ((n.astype(np.float64), a, m, kinv, pose), "uint8, uint16 or float32"),
                       ((n, a.astype(np.uint16), m, kinv, pose), "albedos"),
                       ((n, a[:, :12], m, kinv, pose), "albedos"),
                       ((n[..., :2], None, m, kinv, pose), "normals"),
                       ((n, a, m[:2], kinv, pose), "masks"),
                       ((n, a, m[:, :, :10], kinv, pose), "masks"),
                       ((n, a, m.astype(np.int64), kinv, pose), "masks"),
                       ((n, a, m, kinv[:2], pose), "intrinsics_all_inv"),
                       ((n, a, m, kinv, pose[:, :3]), "pose_all")):
        with pytest.raises(ValueError, match=word):
            make(*args, device="cpu")
    with pytest.raises(ValueError, match="lights"):
        make(n, a, m, kinv, pose, device="cpu", tilt_deg=tuple(range(0, 360, 40)))
    with pytest.raises(RuntimeError, match="GPU"):
        make(torch.from_numpy(n), None, torch.from_numpy(m)[..., None], torch.from_numpy(kinv), pose, device="cpu")


def _plain_rq(m):
    """RQ by a QR decomposition of the row-reversed transpose, signs as they come"""
    flip = np.eye(3)[::-1]
    q, r = np.linalg.qr((flip @ m).T)
    return flip @ r.T @ flip, flip @ q.T


def test_cameras_from_projections_recovers_known_cameras(R):
    """P = K [R | -R C] built from known K, R, C: K / K[2,2] and the pose come back to 1e-6 relative.  At least one of the
    three has a negative diagonal entry in the plain RQ decomposition, so the sign fix is exercised."""
    rng = np.random.default_rng(5)
    Ks, Rs, Cs, world, scale, negative = [], [], [], [], [], 0
    for i in range(3):
        K = np.array([[900.0 + 50 * i, 0.3 * i, 300.0 + i], [0.0, 880.0 - 20 * i, 250.0 - i], [0.0, 0.0, 1.0]]) * (1.0 + 0.5 * i)
        Rm = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        Rm *= np.sign(np.linalg.det(Rm))
        Cc = rng.normal(size=3) * 2.0
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = K @ Rm, -K @ Rm @ Cc
        s = np.diag([1.5, 1.5, 1.5, 1.0])
        s[:3, 3] = (0.1, -0.2, 0.05)
        world.append(P @ np.linalg.inv(s))                     # world_mat @ scale_mat = P
        scale.append(s)
        negative += int((np.diag(_plain_rq((world[-1].astype(np.float32) @ s.astype(np.float32))[:3, :3].astype(np.float64))[0]) < 0).any())
        Ks.append(K / K[2, 2]), Rs.append(Rm), Cs.append(Cc)
    assert negative >= 1, "no camera exercises the sign fix"
    intr, pose = R.cameras_from_projections(world, scale)
    assert intr.shape == (3, 4, 4) and pose.shape == (3, 4, 4) and intr.dtype == torch.float32 and pose.dtype == torch.float32
    # 1e-6 relative to the largest element of each quantity (the float32 product world_mat @ scale_mat and the float32
    # results carry 6e-8 relative each)
    for i in range(3):
        k, p = intr[i].double().numpy(), pose[i].double().numpy()
        assert np.array_equal(k[3], [0, 0, 0, 1]) and np.array_equal(p[3], [0, 0, 0, 1])
        e_k = float(np.abs(k[:3, :3] - Ks[i]).max()) / float(np.abs(Ks[i]).max())
        e_r = float(np.abs(p[:3, :3] - Rs[i].T).max())
        e_c = float(np.abs(p[:3, 3] - Cs[i]).max()) / float(np.abs(Cs[i]).max())
        print(f"SOURCE camera {i}: relative error K {e_k:.2e}, rotation {e_r:.2e}, centre {e_c:.2e}")
        assert e_k <= 1e-6 and e_r <= 1e-6 and e_c <= 1e-6
        assert bool((np.diag(k[:3, :3]) > 0).all()) and k[2, 2] == 1.0 and np.linalg.det(p[:3, :3]) > 0.999
