"""Host-side checks of the whole-image path (no GPU): the interpolated pose of `gen_rays_between` against the pose the
reference built (tests/golden/image_rays_small.npz, tools/gen_image_golden.py), and the argument checks of the two new C
entry points that need no device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.golden_util import POSE_BOUND

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_rays_small.npz")
RNB_E_INVALID, RNB_E_NULL = -1, -4


@pytest.fixture(scope="module")
def R():
    import rnb_neus_fork_amd as pkg
    pkg.native.load()
    return pkg


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLDEN, allow_pickle=False)


def test_interpolated_pose_is_the_references(R, fx):
    """`interpolate_pose` against the pose the reference's gen_rays_between built (its last np.linalg.inv), for ratio 0,
    0.3 and 1.  Measured here on the CPU: largest element difference 0.0 for all three; bound = 4 x measured = 0.0
    (<= 1e-5), i.e. the float32 poses are equal."""
    assert POSE_BOUND <= 1e-5
    seen = []
    for i in range(3):
        i0, i1 = (int(v) for v in fx[f"bt{i}_idx"])
        ratio = float(fx[f"bt{i}_ratio"])
        pose = R.raygen.interpolate_pose(fx["pose_all"][i0], fx["pose_all"][i1], ratio)
        assert pose.dtype == np.float32 and pose.shape == (4, 4)
        diff = float(np.abs(pose.astype(np.float64) - fx[f"bt{i}_pose"].astype(np.float64)).max())
        print(f"IMAGE pose ratio {ratio}: max element difference {diff:.3e} (bound {POSE_BOUND:.3e})")
        assert diff <= POSE_BOUND
        # the reference's rays_o is this pose's translation
        assert np.array_equal(np.broadcast_to(pose[:3, 3], fx[f"bt{i}_rays_o"].shape), fx[f"bt{i}_rays_o"])
        seen.append(ratio)
    assert seen == [0.0, pytest.approx(0.3), 1.0]


def test_ratio_0_and_1_reproduce_the_end_poses(R, fx):
    """Two float32 inversions of a rigid pose with |t| = 3 (condition number about (1 + |t|)^2 = 16) lie within
    2 x 16 x 2^-24 x max|element| = 6e-6 of the pose; the slerp's end points are exact rotations."""
    p0, p2 = fx["pose_all"][0], fx["pose_all"][2]
    bound = 2 * 16 * 2.0 ** -24 * 3.0
    for ratio, want in ((0.0, p0), (1.0, p2)):
        got = R.raygen.interpolate_pose(p0, p2, ratio)
        assert float(np.abs(got - want).max()) <= bound
    half = R.raygen.interpolate_pose(p0, p2, 0.5)
    rot = half[:3, :3].astype(np.float64)
    assert np.allclose(rot @ rot.T, np.eye(3), atol=1e-6) and np.linalg.det(rot) > 0.999
    # the half-way rotation is as far from one end as from the other
    a0 = np.trace(np.linalg.inv(p0)[:3, :3].astype(np.float64).T @ np.linalg.inv(half)[:3, :3])
    a2 = np.trace(np.linalg.inv(p2)[:3, :3].astype(np.float64).T @ np.linalg.inv(half)[:3, :3])
    assert abs(a0 - a2) < 1e-5


def test_slerp_is_the_scaled_relative_rotation(R):
    """R0 exp(t log(R0^T R1)) on rotations about one axis: the angle interpolates linearly, also beyond 90 degrees and
    through the quaternion's largest-component branches."""
    def rz(a):
        return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    tilt = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    for a0, a1 in ((0.1, 2.9), (-3.0, -0.2), (2.0, 2.0), (3.0, 3.1)):
        for t in (0.0, 0.25, 0.7, 1.0):
            got = R.raygen._slerp(tilt @ rz(a0), tilt @ rz(a1), t)
            assert np.allclose(got, tilt @ rz(a0 + t * (a1 - a0)), atol=1e-12), (a0, a1, t)


def test_fixture_grid_is_torch_linspace(fx):
    """the coordinates the Python side hands to rnb_gen_rays_grid are the reference's, bit for bit; level 2 has the
    half-way rows 2.5 and 7.5"""
    H, W = fx["images"].shape[2:4]
    for i in range(3):
        l = int(fx[f"at{i}_level"])
        tx, ty = torch.linspace(0, W - 1, W // l), torch.linspace(0, H - 1, H // l)
        assert np.array_equal(fx[f"at{i}_pixels_x"], tx[None, :].expand(H // l, W // l).numpy())
        assert np.array_equal(fx[f"at{i}_pixels_y"], ty[:, None].expand(H // l, W // l).numpy())
    assert [float(v) for v in fx["at1_pixels_y"][:, 0]] == [0.0, 2.5, 5.0, 7.5, 10.0]
    assert [int(v) for v in torch.from_numpy(fx["at1_pixels_y"][:, 0]).round().long()] == [0, 2, 5, 8, 10]


def _desc(R):
    from rnb_neus_fork_amd.fields import SDFNetwork, RenderingNetwork, model_desc
    sdf = SDFNetwork(d_in=3, d_out=65, d_hidden=64, n_layers=4, skip_in=(2,), multires=6)
    col = RenderingNetwork(d_feature=64, mode="no_view_dir", d_in=6, d_out=3, d_hidden=64, n_layers=2, multires_view=4)
    return model_desc(sdf, col, 16, 16, 4)


def test_render_maps_argument_checks_need_no_device(R):
    """refusals that come before the first HIP call: NULL structs, RNB_FLAG_INPUT_GRADS, no map, S = 513, 9 lights"""
    lib, N = R.native.load(), R.native
    desc = _desc(R)
    host = (C.c_float * 64)()
    fake = C.c_void_p(C.addressof(host))     # never dereferenced: every case below is refused first
    a, m = N.RenderArgs(), N.RenderMapsOut()
    a.B, a.S, a.n_lights, a.flags = 4, 32, 3, N.MODE_MVPS
    for f in ("rays_o", "rays_d", "z_vals", "lights_dir", "variance"):
        setattr(a, f, fake.value)

    def call():
        rc = lib.rnb_render_maps(C.byref(desc), fake, C.byref(a), C.byref(m), fake, 1 << 40, None)
        return rc, lib.rnb_last_error_string().decode()

    assert lib.rnb_render_maps(C.byref(desc), None, C.byref(a), C.byref(m), fake, 0, None) == RNB_E_NULL
    assert lib.rnb_render_maps(C.byref(desc), fake, C.byref(a), None, fake, 0, None) == RNB_E_NULL
    rc, msg = call()
    assert rc == RNB_E_INVALID and "no map" in msg
    m.color = fake.value
    a.flags = N.MODE_MVPS | N.FLAG_INPUT_GRADS
    rc, msg = call()
    assert rc == RNB_E_INVALID and "INPUT_GRADS" in msg
    a.flags, a.S = N.MODE_MVPS, 513
    rc, msg = call()
    assert rc == RNB_E_INVALID and "kMaxS" in msg
    a.S, a.n_lights = 32, 9
    rc, msg = call()
    assert rc == RNB_E_INVALID and "kMaxRenderLights" in msg
    a.n_lights, a.flags = 3, N.MODE_MVPS | N.FLAG_NO_ALBEDO
    m.albedo = fake.value
    rc, msg = call()
    assert rc == RNB_E_INVALID and "albedo" in msg
    a.flags = N.MODE_CORE
    rc, msg = call()
    assert rc == RNB_E_INVALID and "albedo" in msg


def test_gen_rays_grid_argument_checks_need_no_device(R):
    lib = R.native.load()
    host = (C.c_float * 64)()
    fake = C.c_void_p(C.addressof(host))

    def call(first=0, n=40, light=-1, rgb=None, images=None, tx=fake, Wl=8, Hl=5):
        rc = lib.rnb_gen_rays_grid(fake, fake, tx, fake, Wl, Hl, first, n, images, None, fake, 1, None, 3, light, 11, 16, fake,
                                   rgb, None, None, None, None, None)
        return rc, lib.rnb_last_error_string().decode()

    assert call(tx=None)[0] == RNB_E_NULL
    assert call(rgb=fake)[0] == RNB_E_NULL                      # true_rgb without images
    for kw, word in ((dict(first=1, n=40), "outside"), (dict(first=-1, n=4), "outside"), (dict(n=0), "outside"),
                     (dict(light=3), "light"), (dict(light=-2), "light"), (dict(Wl=0), "bad shape")):
        rc, msg = call(**kw)
        assert rc == RNB_E_INVALID and word in msg, (kw, rc, msg)
