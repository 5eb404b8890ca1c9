"""Host-side checks of camera refinement (no GPU): `rnb_gen_rays_camera_bwd` is declared, exported and bound, and refuses
bad arguments before it touches a device; `CameraRefinement.camera` in fp32 against the fp64 restatement of
tests/camera_refine_util.py by the output rule of tests/parity.py over rotations from 0 to 3 rad; value and gradient at
w = 0; the zero correction reproduces the stored camera bit for bit; refined poses stay rigid."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import camera_refine_util as CU
from tests.parity import check_value, rel_l2

RNB_E_INVALID, RNB_E_NULL = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLES = [0.0, 1e-8, 1e-4, 1e-3, 0.3, 3.0]


@pytest.fixture(scope="module")
def R():
    import rnb_neus_fork_amd as pkg
    pkg.native.load()
    return pkg


@pytest.fixture(scope="module")
def cams():
    ds = CU.stack_fixture()
    return ds["pose_all"], ds["intrinsics_all_inv"]


def test_symbol_is_declared_exported_and_bound(R):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnbneus.h")).read(), flags=re.S)
    assert re.search(r"\brnb_gen_rays_camera_bwd\s*\(", text), "not declared in include/rnbneus.h"
    assert "rnb_gen_rays_camera_bwd" in R.native.EXPORTED_SYMBOLS
    lib = R.native.load()
    fn = lib.rnb_gen_rays_camera_bwd
    assert fn.restype is C.c_int and len(fn.argtypes) == 15
    assert fn.argtypes[4] is C.c_int64 and fn.argtypes[6] is C.c_int32
    assert lib.rnb_abi_version() == 5 and R.native.ABI_VERSION == 5
    assert R.CameraRefinement is R.camera_refine.CameraRefinement and "CameraRefinement" in R.__all__


def test_argument_checks_need_no_device(R):
    """every refusal comes before the first HIP call: the pointers are host addresses that are never dereferenced"""
    lib = R.native.load()
    host = (C.c_float * 64)()
    fake = C.c_void_p(C.addressof(host))

    def call(kinv=fake, pose=fake, px=fake, py=fake, B=4, lights=None, L=0, lights_bar=None, pose_bar=fake):
        rc = lib.rnb_gen_rays_camera_bwd(kinv, pose, px, py, B, lights, L, fake, fake, lights_bar, None, None, pose_bar,
                                         None, None)
        return rc, lib.rnb_last_error_string().decode()

    for kw in (dict(kinv=None), dict(pose=None), dict(px=None), dict(py=None), dict(pose_bar=None),
               dict(lights_bar=fake, L=3)):
        rc, msg = call(**kw)
        assert rc == RNB_E_NULL and "rnb_gen_rays_camera_bwd" in msg, (kw, rc, msg)
    for kw, word in ((dict(B=0), "shape"), (dict(B=-3), "shape"), (dict(L=-1), "n_lights"), (dict(L=9), "n_lights"),
                     (dict(lights=fake, L=0), "n_lights"), (dict(lights=fake, lights_bar=fake, L=9), "n_lights")):
        rc, msg = call(**kw)
        assert rc == RNB_E_INVALID and word in msg, (kw, rc, msg)


def _direction(seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(3, generator=g, dtype=torch.float64)
    return u / u.norm()


@pytest.mark.parametrize("angle", ANGLES)
def test_camera_fp32_against_fp64(R, cams, angle):
    pose_all, kinv_all = cams
    V = pose_all.shape[0]
    ref = R.CameraRefinement(V, refine_focal=True)
    for v in range(V):
        w = _direction(10 + v) * angle
        tau = torch.tensor([0.02, -0.01, 0.03], dtype=torch.float64) * (v + 1)
        s = torch.tensor(0.05 * (v - 1), dtype=torch.float64)
        with torch.no_grad():
            ref.pose_delta[v] = torch.cat([w, tau]).float()
            ref.focal_log_scale[v] = s.float()
        # the references see the float32 parameter values the module holds
        d32, s32 = ref.pose_delta[v].detach(), ref.focal_log_scale[v].detach()
        p64, k64, _ = CU.camera(d32.double(), s32.double(), pose_all[v].double(), kinv_all[v].double())
        p32, k32, _ = CU.camera(d32, s32, pose_all[v], kinv_all[v])
        pose, kinv = ref.camera(v, pose_all[v], kinv_all[v])
        assert pose.dtype == torch.float32 and kinv.dtype == torch.float32
        print(f"angle {angle:g} view {v}: pose {check_value('pose', pose, p64, p32):.2f} of its bound, "
              f"intrinsics_inv {check_value('intrinsics_inv', kinv, k64, k32):.2f}")
        assert torch.equal(pose[3], pose_all[v][3]) and torch.equal(kinv[2:], kinv_all[v][2:])
        e64 = CU.so3_exp(d32[:3].double())
        check_value("rotation", ref.rotation(v), e64, CU.so3_exp(d32[:3]))
    # all views at once are the same cameras
    poses, kinvs = ref.poses(pose_all), ref.intrinsics_inv(kinv_all)
    for v in range(V):
        pose, kinv = ref.camera(v, pose_all[v], kinv_all[v])
        assert torch.equal(poses[v], pose) and torch.equal(kinvs[v], kinv)


def test_value_and_gradient_are_finite_at_zero(R, cams):
    pose_all, kinv_all = cams
    ref = R.CameraRefinement(pose_all.shape[0], refine_focal=True)
    g = torch.Generator().manual_seed(3)
    wp, wk = torch.randn(4, 4, generator=g), torch.randn(4, 4, generator=g)
    pose, kinv = ref.camera(1, pose_all[1], kinv_all[1])
    ((pose * wp).sum() + (kinv * wk).sum()).backward()
    assert bool(torch.isfinite(pose).all()) and bool(torch.isfinite(kinv).all())
    gd, gs = ref.pose_delta.grad, ref.focal_log_scale.grad
    assert bool(torch.isfinite(gd).all()) and bool(torch.isfinite(gs).all())
    assert bool((gd[0] == 0).all()) and bool((gd[2] == 0).all()) and float(gs[0]) == 0.0 and float(gs[2]) == 0.0
    d = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    s = torch.zeros((), dtype=torch.float64, requires_grad=True)
    p64, k64, _ = CU.camera(d, s, pose_all[1].double(), kinv_all[1].double())
    ((p64 * wp.double()).sum() + (k64 * wk.double()).sum()).backward()
    assert float(d.grad[:3].norm()) > 0.1 and float(d.grad[3:].norm()) > 0.1 and abs(float(s.grad)) > 1e-3
    assert rel_l2(gd[1], d.grad) <= 1e-6 and rel_l2(gs[1], s.grad) <= 1e-6


@pytest.mark.parametrize("refine_focal", [False, True])
def test_zero_correction_is_the_stored_camera_bit_for_bit(R, cams, refine_focal):
    pose_all, kinv_all = cams
    ref = R.CameraRefinement(pose_all.shape[0], refine_focal=refine_focal)
    assert tuple(ref.pose_delta.shape) == (3, 6) and not bool(ref.pose_delta.any())
    assert (ref.focal_log_scale is not None) == refine_focal
    assert len(list(ref.parameters())) == (2 if refine_focal else 1)
    for v in range(pose_all.shape[0]):
        pose, kinv = ref.camera(v, pose_all[v], kinv_all[v])
        assert torch.equal(pose, pose_all[v]) and torch.equal(kinv, kinv_all[v])
        assert torch.equal(ref.rotation(v), torch.eye(3))
    assert torch.equal(ref.poses(pose_all), pose_all) and torch.equal(ref.intrinsics_inv(kinv_all), kinv_all)
    with pytest.raises(IndexError):
        ref.camera(3, pose_all[0], kinv_all[0])
    with pytest.raises(ValueError):
        ref.poses(pose_all[:2])


def test_refined_poses_stay_orthonormal(R, cams):
    pose_all, _ = cams
    V = pose_all.shape[0]
    ref = R.CameraRefinement(V)
    eye = torch.eye(3, dtype=torch.float64)
    with torch.no_grad():
        for v, angle in enumerate((1e-3, 0.3, 3.0)):
            ref.pose_delta[v, :3] = (_direction(20 + v) * angle).float()
    poses = ref.poses(pose_all).detach().double()
    for v in range(V):
        r0, r1 = pose_all[v, :3, :3].double(), poses[v, :3, :3]
        stored = float((r0 @ r0.T - eye).abs().max())
        # Exp(w) in fp32 is orthonormal to a few ulps and the product adds a 3-term sum's rounding: 16 x 2^-24 over the stored error
        bound = stored + 16 * 2.0 ** -24
        err = float((r1 @ r1.T - eye).abs().max())
        print(f"view {v}: |R R^T - I| {err:.2e} (stored {stored:.2e}, bound {bound:.2e})")
        assert err <= bound and float(torch.linalg.det(r1)) > 0.999
