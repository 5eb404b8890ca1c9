"""Camera refinement on the device: `rnb_gen_rays_camera_bwd` (the backward of `DeviceRays.sample` in its camera) against
fp64 torch autograd through the restatement of tests/camera_refine_util.py, its contracts (zero border, omitted adjoints,
bit-reproducibility), the forward with `set_refinement`, and whole steps (`sample` -> render -> loss -> backward) whose
`pose_delta` / `focal_log_scale` gradients are compared with fp64 autograd through oracle/rnb_oracle.py on the
restatement's rays and the device's own depths.  Stack mode is tests/golden/raygen_small.npz (20 x 24), source mode the
u8 maps of tests/golden/source_maps_small.npz (13 x 11).

As in tests/test_gpu_render_input_grads.py the oracle runs with a graph-keeping normal (the reference's gradient() keeps
the graph to the points), and the random functional + loss of that file is restated here."""
from dataclasses import replace

import pytest
import torch

from oracle import rnb_oracle as O
from tests import camera_refine_util as CU
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device
from tests.oracle_normal import graph_normal  # noqa: F401
from tests.parity import GRAD_CAP, K_GRAD, check_grad, check_value, grad_bound, rel_l2
from tests.ray_matrix import FLOAT_OUTS
from tests.shape_matrix import BY_NAME, live_params

pytestmark = pytest.mark.gpu

VIEW = {"stack": 1, "source": 0}       # the views of the two fixtures that look at the origin most squarely
SIZES = [1, 63, 64, 65, 333, 1000]     # a lone ray, both sides of a wave, a tail, several strides of the 256-lane workgroup
DELTA = torch.tensor([0.006, -0.008, 0.005, 0.01, -0.007, 0.012])     # |w| ~ 1e-2 rad, |tau| ~ 1e-2
LOG_SCALE = torch.tensor(0.05)


@pytest.fixture(scope="module")
def rigs(R):
    """mode -> dict(dr, pose [V,4,4], kinv [V,4,4], H, W, lights: what the mode's per-ray lights are made from)"""
    ds, fx = CU.stack_fixture(), CU.source_fixture()
    stack = R.DeviceRays(ds["images"], ds["images_warmup"], ds["masks"], ds["light_directions"],
                         ds["light_directions_warmup"], ds["intrinsics_all_inv"], ds["pose_all"], device())
    kinv, pose = torch.from_numpy(fx["intrinsics_inv"]), torch.from_numpy(fx["pose"])
    source = R.DeviceRays.from_source_maps(fx["normals_u8"], fx["albedo_u8"], fx["masks_u8"], kinv, pose, device())
    return {"stack": dict(dr=stack, pose=ds["pose_all"], kinv=ds["intrinsics_all_inv"], H=20, W=24,
                          lights=ds["light_directions"], warm=ds["light_directions_warmup"]),
            "source": dict(dr=source, pose=pose, kinv=kinv, H=13, W=11, lights=torch.from_numpy(fx["l_cam"]),
                           warm=source.light_directions_warmup.cpu())}


def _restated(rig, mode, v, px, py, delta, s, dt, warmup=False):
    """What `sample` returns for view `v` under the correction (delta, s), in dtype dt, with a graph to delta and s."""
    pose, kinv, E = CU.camera(delta, s, rig["pose"][v].to(dt), rig["kinv"][v].to(dt))
    o, d, near, far = CU.rays(kinv, pose, px, py)
    L = rig["lights"].shape[1]
    if warmup:
        lights = CU.rotate(rig["warm"][v].to(dt), E).reshape(L, 1, 1, 3)
    else:
        per_pixel = rig["lights"][v][:, py, px].to(dt)                        # [L,B,3]
        lights = CU.rotate(per_pixel, pose[:3, :3] if mode == "source" else E).reshape(L, -1, 1, 3)
    return {"rays_o": o, "rays_d": d, "near": near, "far": far, "lights_dir": lights}, pose, kinv


def _adjoints(B, L, seed, keys=("rays_o", "rays_d", "near", "far", "lights_dir")):
    g = torch.Generator().manual_seed(seed)
    shapes = {"rays_o": (B, 3), "rays_d": (B, 3), "near": (B, 1), "far": (B, 1), "lights_dir": (L, B, 1, 3)}
    return {k: (torch.randn(shapes[k], generator=g, dtype=torch.float64) if k in keys else None) for k in shapes}


def _camera_of(rig, v):
    """the fp32 refined camera of view v the kernel tests differentiate in (leaf tensors)"""
    with torch.no_grad():
        pose, kinv, _ = CU.camera(DELTA, LOG_SCALE, rig["pose"][v], rig["kinv"][v])
    return pose.contiguous(), kinv.contiguous()


def _device_camera_grads(rig, v, px, py, pose, kinv, adj):
    dr = rig["dr"]
    pd, kd = pose.to(device()).requires_grad_(True), kinv.to(device()).requires_grad_(True)
    s = dr.sample(v, px.numel(), pixels_x=px, pixels_y=py, pose=pd, intrinsics_inv=kd)
    for k in ("mask", "true_rgb", "pixels_x", "pixels_y"):
        assert not s[k].requires_grad, f"{k} must not carry a graph"
    for k in ("rays_o", "rays_d", "near", "far"):
        assert s[k].requires_grad, f"{k} must carry a graph"
    CU.adjoint_loss(s, {k: (None if g is None else g.to(device())) for k, g in adj.items()}).backward()
    torch.cuda.synchronize()
    return pd.grad, kd.grad, s


def _reference_camera_grads(rig, mode, v, px, py, pose, kinv, adj, dt):
    p, k = pose.to(dt).requires_grad_(True), kinv.to(dt).requires_grad_(True)
    o, d, near, far = CU.rays(k, p, px, py)
    out = {"rays_o": o, "rays_d": d, "near": near, "far": far}
    if mode == "source":
        L = rig["lights"].shape[1]
        out["lights_dir"] = CU.rotate(rig["lights"][v][:, py, px].to(dt), p[:3, :3]).reshape(L, -1, 1, 3)
    CU.adjoint_loss(out, {k_: g for k_, g in adj.items() if k_ in out}).backward()
    zero = torch.zeros(4, 4, dtype=dt)
    return (zero if p.grad is None else p.grad), (zero if k.grad is None else k.grad)


def _check_camera_grads(tag, got, g64, g32):
    for name, mine, r64, r32 in (("pose", got[0], g64[0], g32[0]), ("intrinsics_inv", got[1], g64[1], g32[1])):
        mine = mine.cpu()
        assert bool(torch.isfinite(mine).all()), f"{tag} {name}: not finite"
        assert float(r64.norm()) > 0.0, f"{tag} {name}: the fp64 gradient vanishes: not a parity target"
        rel32 = rel_l2(r32, r64)
        print(f"{tag} {name}.grad: |g64| {float(r64.norm()):.3g}, rel-L2 {rel_l2(mine, r64):.2e} "
              f"(fp32 autograd {rel32:.2e}, bound {grad_bound(rel32):.2e})")
        check_grad(f"{tag} {name}", mine, r64, rel32)
    assert bool((got[0][3] == 0).all()), f"{tag}: pose.grad's last row is not exactly 0"
    assert bool((got[1][3] == 0).all()) and bool((got[1][:, 3] == 0).all()), \
        f"{tag}: intrinsics_inv.grad outside [:3,:3] is not exactly 0"


# ------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("mode", ["stack", "source"])
def test_camera_adjoint_against_fp64(R, rigs, mode, B):
    rig, v = rigs[mode], VIEW[mode]
    px, py = CU.pixels(B, rig["H"], rig["W"], seed=100 + B)
    if B > 1:
        assert len(torch.unique(py * rig["W"] + px)) < B, "the pixels must contain duplicates"
    pose, kinv = _camera_of(rig, v)
    adj = _adjoints(B, rig["lights"].shape[1], seed=7 * B)
    got_p, got_k, s = _device_camera_grads(rig, v, px, py, pose, kinv, adj)
    assert s["lights_dir"].requires_grad == (mode == "source"), "stack-mode lights are gathers: no graph to the pose"
    g64 = _reference_camera_grads(rig, mode, v, px, py, pose, kinv, adj, torch.float64)
    g32 = _reference_camera_grads(rig, mode, v, px, py, pose, kinv, adj, torch.float32)
    _check_camera_grads(f"{mode} B={B}", (got_p, got_k), g64, g32)


@pytest.mark.parametrize("keys", [("rays_o",), ("rays_d",), ("near",), ("far",), ("lights_dir",), ("rays_d", "far")],
                         ids=lambda k: "+".join(k))
def test_omitted_adjoints_are_zeros(R, rigs, keys):
    """through autograd an output that is not used sends no adjoint at all (NULL at the entry point)"""
    rig, v, B = rigs["source"], VIEW["source"], 65
    px, py = CU.pixels(B, rig["H"], rig["W"], seed=41)
    pose, kinv = _camera_of(rig, v)
    adj = _adjoints(B, 3, seed=43, keys=keys)
    got_p, got_k, _ = _device_camera_grads(rig, v, px, py, pose, kinv, adj)
    g64 = _reference_camera_grads(rig, "source", v, px, py, pose, kinv, adj, torch.float64)
    g32 = _reference_camera_grads(rig, "source", v, px, py, pose, kinv, adj, torch.float32)
    tag = "only " + "+".join(keys)
    if keys in (("rays_o",), ("lights_dir",)):       # rays_o = t and the lights do not depend on the intrinsics
        assert float(g64[1].abs().max()) == 0.0 and not bool(got_k.any()), f"{tag}: intrinsics_inv.grad must be exactly 0"
        check_grad(f"{tag} pose", got_p.cpu(), g64[0], rel_l2(g32[0], g64[0]))
    else:
        _check_camera_grads(tag, (got_p, got_k), g64, g32)


def test_entry_point_takes_null_for_zero(R, rigs):
    """the entry point itself: NULL adjoints give the bits that explicit zeros give, and NULL intrinsics_inv_bar is allowed"""
    rig, v, B, L = rigs["source"], VIEW["source"], 333, 3
    lib, ptr, dev = R.native.load(), R.native.ptr, device()
    px, py = (t.to(dev) for t in CU.pixels(B, rig["H"], rig["W"], seed=5))
    pose, kinv = (t.to(dev) for t in _camera_of(rig, v))
    adj = {k: g.float().to(dev).contiguous() for k, g in _adjoints(B, L, seed=9).items()}
    lights = rig["dr"].sample(v, B, pixels_x=px, pixels_y=py, pose=pose, intrinsics_inv=kinv)["lights_dir"].reshape(L, B, 3)
    lights = lights.contiguous()

    def run(o=None, d=None, lb=None, near=None, far=None, want_k=True, with_lights=True):
        pb = torch.full((4, 4), float("nan"), device=dev)
        kb = torch.full((4, 4), float("nan"), device=dev) if want_k else None
        R.native.check(lib.rnb_gen_rays_camera_bwd(ptr(kinv), ptr(pose), ptr(px), ptr(py), B,
                                                   ptr(lights) if with_lights else None, L if with_lights else 0, ptr(o),
                                                   ptr(d), ptr(lb), ptr(near), ptr(far), ptr(pb), ptr(kb), None))
        torch.cuda.synchronize()
        return pb, kb

    z3, z1, zl = torch.zeros(B, 3, device=dev), torch.zeros(B, device=dev), torch.zeros(L, B, 3, device=dev)
    full = run(adj["rays_o"], adj["rays_d"], adj["lights_dir"], adj["near"].reshape(B), adj["far"].reshape(B))
    assert bool(torch.isfinite(full[0]).all()) and bool(torch.isfinite(full[1]).all()), "an entry was left unwritten"
    a = run(d=adj["rays_d"])
    b = run(z3, adj["rays_d"], zl, z1, z1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = run(d=adj["rays_d"], with_lights=False)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    none = run()
    assert not bool(none[0].any()) and not bool(none[1].any())
    only_pose = run(adj["rays_o"], adj["rays_d"], adj["lights_dir"], adj["near"].reshape(B), adj["far"].reshape(B), want_k=False)
    assert only_pose[1] is None and torch.equal(only_pose[0], full[0])


def test_a_camera_that_requires_grad_must_live_on_the_device(R, rigs):
    """its gradient is made on the device in float32: a host or float64 leaf is refused in sample(), not in the backward"""
    rig, v = rigs["source"], VIEW["source"]
    px, py = CU.pixels(8, rig["H"], rig["W"], seed=1)
    pose, kinv = _camera_of(rig, v)
    for bad in (pose.clone().requires_grad_(True), pose.double().to(device()).requires_grad_(True)):
        with pytest.raises(ValueError, match="requires grad"):
            rig["dr"].sample(v, 8, pixels_x=px, pixels_y=py, pose=bad)
    s = rig["dr"].sample(v, 8, pixels_x=px, pixels_y=py, pose=pose, intrinsics_inv=kinv)     # without grad a host matrix is moved
    assert not s["rays_d"].requires_grad and bool(torch.isfinite(s["rays_d"]).all())


@pytest.mark.parametrize("mode", ["stack", "source"])
def test_camera_adjoint_is_bit_reproducible(R, rigs, mode):
    rig, v, B = rigs[mode], VIEW[mode], 1000
    px, py = CU.pixels(B, rig["H"], rig["W"], seed=100 + B)
    pose, kinv = _camera_of(rig, v)
    adj = _adjoints(B, 3, seed=7 * B)
    p1, k1, _ = _device_camera_grads(rig, v, px, py, pose, kinv, adj)
    p2, k2, _ = _device_camera_grads(rig, v, px, py, pose, kinv, adj)
    assert torch.equal(p1, p2) and torch.equal(k1, k2)


# ------------------------------------------------------------------------------------------------------------ the forward
def _same(a, b, tag):
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), f"{tag}: {k} differs"
        else:
            assert a[k] == b[k], f"{tag}: {k} differs"


@pytest.mark.parametrize("mode", ["stack", "source"])
def test_zero_refinement_changes_no_bit(R, rigs, mode):
    rig, v = rigs[mode], VIEW[mode]
    dr = rig["dr"]
    px, py = CU.pixels(65, rig["H"], rig["W"], seed=3)
    calls = {"sample": lambda: dr.sample(v, 65, pixels_x=px, pixels_y=py),
             "sample warmup": lambda: dr.sample(v, 65, warmup=True, pixels_x=px, pixels_y=py),
             "view_rays": lambda: dr.view_rays(v), "view_rays light 1": lambda: dr.view_rays(v, light=1, first=7, count=50),
             "view_rays warmup": lambda: dr.view_rays(v, warmup=True, resolution_level=2)}
    plain = {k: f() for k, f in calls.items()}
    assert not plain["sample"]["rays_d"].requires_grad
    dr.set_refinement(R.CameraRefinement(3, refine_focal=True).to(device()))
    try:
        refined = {k: f() for k, f in calls.items()}
        with torch.no_grad():
            quiet = dr.sample(v, 65, pixels_x=px, pixels_y=py)
    finally:
        dr.set_refinement(None)
    for k in calls:
        _same(plain[k], refined[k], f"{mode} {k}")
    _same(plain["sample"], quiet, f"{mode} sample under no_grad")
    assert refined["sample"]["rays_d"].requires_grad and not quiet["rays_d"].requires_grad
    assert not refined["view_rays"]["rays_d"].requires_grad, "view_rays is forward only"
    with pytest.raises(ValueError, match="views"):
        dr.set_refinement(R.CameraRefinement(4))


def _refinement(R, v, focal=True, delta=DELTA, log_scale=LOG_SCALE):
    ref = R.CameraRefinement(3, refine_focal=focal)
    with torch.no_grad():
        ref.pose_delta[v] = delta
        if focal:
            ref.focal_log_scale[v] = log_scale
    return ref.to(device())


@pytest.mark.parametrize("mode", ["stack", "source"])
def test_refined_forward_against_fp64(R, rigs, mode):
    rig, v = rigs[mode], VIEW[mode]
    dr = rig["dr"]
    B = 65
    px, py = CU.pixels(B, rig["H"], rig["W"], seed=3)
    dr.set_refinement(_refinement(R, v))
    try:
        got = {False: dr.sample(v, B, pixels_x=px, pixels_y=py), True: dr.sample(v, B, warmup=True, pixels_x=px, pixels_y=py)}
        whole = dr.view_rays(v)
    finally:
        dr.set_refinement(None)
    plain = dr.sample(v, B, pixels_x=px, pixels_y=py)
    assert torch.equal(got[False]["true_rgb"], plain["true_rgb"]) and torch.equal(got[False]["mask"], plain["mask"])
    assert not torch.equal(got[False]["rays_d"], plain["rays_d"]) and not torch.equal(got[False]["lights_dir"], plain["lights_dir"])
    for warmup in (False, True):
        r64, _, _ = _restated(rig, mode, v, px, py, DELTA.double(), LOG_SCALE.double(), torch.float64, warmup)
        r32, _, _ = _restated(rig, mode, v, px, py, DELTA, LOG_SCALE, torch.float32, warmup)
        for k in r64:
            frac = check_value(f"{mode} warmup={warmup} {k}", got[warmup][k], r64[k], r32[k])
            print(f"{mode} warmup={warmup} {k}: {frac:.2f} of its bound")
    # the whole view runs on the same camera
    ys, xs = torch.meshgrid(torch.arange(rig["H"]), torch.arange(rig["W"]), indexing="ij")
    ax, ay = xs.reshape(-1), ys.reshape(-1)
    r64, _, _ = _restated(rig, mode, v, ax, ay, DELTA.double(), LOG_SCALE.double(), torch.float64)
    r32, _, _ = _restated(rig, mode, v, ax, ay, DELTA, LOG_SCALE, torch.float32)
    for k in r64:
        check_value(f"{mode} view_rays {k}", whole[k], r64[k], r32[k])


def _build(R, name, render=None):
    shape = BY_NAME[name]
    mc = shape.mc if render is None else replace(shape.mc, render=render)
    p = live_params(mc, shape.seed)
    sdf, devn, col, ren = R.build_from_named_params(mc, p, device())
    return mc, p, sdf, devn, col, ren


def test_render_image_runs_on_the_refined_view(R, rigs):
    rig, v = rigs["source"], VIEW["source"]
    dr = rig["dr"]
    mc, p, sdf, devn, col, ren = _build(R, "default_64x64", render=O.RenderConf(n_samples=16, n_importance=16))
    plain = ren.render_image(dr, v, perturb_overwrite=0)
    dr.set_refinement(_refinement(R, v, delta=DELTA * 3))
    try:
        moved = ren.render_image(dr, v, perturb_overwrite=0)
    finally:
        dr.set_refinement(None)
    assert moved["color"].shape == plain["color"].shape == (3, 13, 11, 3)
    assert bool(torch.isfinite(moved["color"]).all()) and float(moved["weight_sum"].max()) > 0.5
    assert torch.equal(moved["true_rgb"], plain["true_rgb"]), "targets belong to the pixels, not to the camera"
    assert not torch.equal(moved["weight_sum"], plain["weight_sum"]), "the refined camera must move the image"


# ------------------------------------------------------------------------------------------------------------ whole steps
B_STEP = 64


def _functional(out, seed=5):
    """A fixed random linear functional of every float output (scaled to O(1) per tensor)."""
    g = torch.Generator().manual_seed(seed)
    total = 0.0
    for k in FLOAT_OUTS:
        t = out[k]
        w = torch.randn(tuple(t.shape), generator=g, dtype=torch.float64) / max(1, t.numel()) ** 0.5
        total = total + (w.to(t.device, t.dtype) * t).sum()
    return total


def _loss(out, true_rgb, mask):
    return _functional(out) + O.rnb_loss(out, true_rgb, mask)[0]


def _oracle_step(p, mc, rig, mode, v, px, py, delta, log_scale, warmup, z, t_rand, true_rgb, mask, dt):
    """(d loss / d delta [6], d loss / d log_scale) by torch autograd in dtype dt: restated rays -> oracle render -> loss"""
    q = {k: t.to(dt).detach().requires_grad_(True) for k, t in p.items()}
    d, s = delta.to(dt).detach().requires_grad_(True), log_scale.to(dt).detach().requires_grad_(True)
    with torch.enable_grad():
        x, _, _ = _restated(rig, mode, v, px, py, d, s, dt, warmup)
        out = O.render_rnb(q, mc, x["rays_o"], x["rays_d"], x["near"], x["far"], x["lights_dir"], cos_anneal_ratio=0.5,
                           warmup=warmup, z_vals=None if z is None else z.to(dt), t_rand=None if t_rand is None else t_rand.to(dt))
        _loss(out, true_rgb.to(dt), mask.to(dt)).backward()
    return d.grad, s.grad


def _device_step(R, ren, rig, v, px, py, delta, log_scale, warmup, t_rand):
    dr = rig["dr"]
    ref = _refinement(R, v, delta=delta, log_scale=log_scale)
    dr.set_refinement(ref)
    try:
        s = dr.sample(v, px.numel(), warmup=warmup, pixels_x=px, pixels_y=py)
        fn = ren.render_rnb_warmup if warmup else ren.render_rnb
        out = fn(s["rays_o"], s["rays_d"], s["near"], s["far"], s["lights_dir"], cos_anneal_ratio=0.5,
                 t_rand=None if t_rand is None else t_rand.to(device()), perturb_overwrite=-1 if t_rand is not None else 0)
        _loss(out, s["true_rgb"], s["mask"]).backward()
        torch.cuda.synchronize()
    finally:
        dr.set_refinement(None)
    return ref, s, out


def _check_step(tag, ref, v, g64, g32):
    for name, mine, r64, r32 in (("pose_delta", ref.pose_delta.grad, g64[0], g32[0]),
                                 ("focal_log_scale", ref.focal_log_scale.grad, g64[1].reshape(1), g32[1].reshape(1))):
        assert mine is not None, f"{tag} {name}: no gradient"
        mine = mine.cpu()
        own = mine[v].reshape(r64.shape)
        assert bool(torch.isfinite(mine).all()), f"{tag} {name}: not finite"
        assert float(r64.norm()) > 0.0, f"{tag} {name}: the fp64 gradient vanishes: not a parity target"
        rel32 = rel_l2(r32, r64)
        print(f"{tag} {name}.grad[{v}]: fp64 {r64.tolist()}, rel-L2 {rel_l2(own, r64):.2e} "
              f"(fp32 oracle {rel32:.2e}, bound {grad_bound(rel32):.2e})")
        assert rel32 < GRAD_CAP / K_GRAD, f"{tag} {name}: the fp32 oracle itself is {rel32:.2e} from fp64: not a parity target"
        check_grad(f"{tag} {name}", own, r64, rel32)
        others = [u for u in range(mine.shape[0]) if u != v]
        assert not bool(mine[others].any()), f"{tag} {name}: the other views' rows are not exactly 0"


STEPS = [("source", False, True), ("stack", False, True), ("source", True, True), ("stack", True, True),
         ("source", False, False)]


@pytest.mark.parametrize("mode,warmup,moved", STEPS,
                         ids=[f"{m}-{'warmup' if w else 'rnb'}-{'moved' if d else 'zero'}" for m, w, d in STEPS])
def test_step_gradients_against_fp64(R, rigs, graph_normal, mode, warmup, moved):
    rig, v = rigs[mode], VIEW[mode]
    mc, p, sdf, devn, col, ren = _build(R, "default_64x64")
    px, py = CU.surface_pixels(rig["kinv"][v], rig["pose"][v], rig["H"], rig["W"], B_STEP, seed=17)
    delta, log_scale = (DELTA, LOG_SCALE) if moved else (torch.zeros(6), torch.zeros(()))
    ref, s, out = _device_step(R, ren, rig, v, px, py, delta, log_scale, warmup, None)
    assert float(out["weight_sum"].detach().mean()) > 0.3, "degenerate scene: rays do not hit a surface"
    z, rgb, mask = ren.last_z_vals.cpu(), s["true_rgb"].detach().cpu(), s["mask"].detach().cpu()
    torch.set_num_threads(16)
    g64 = _oracle_step(p, mc, rig, mode, v, px, py, delta, log_scale, warmup, z, None, rgb, mask, torch.float64)
    g32 = _oracle_step(p, mc, rig, mode, v, px, py, delta, log_scale, warmup, z, None, rgb, mask, torch.float32)
    _check_step(f"{mode} {'warmup' if warmup else 'rnb'} {'moved' if moved else 'zero'}", ref, v, g64, g32)


def test_step_with_live_near_far(R, rigs, graph_normal):
    """n_importance = 0: the depths are near + (far - near) u, so the near / far adjoints reach the camera"""
    rig, v, mode = rigs["source"], VIEW["source"], "source"
    mc, p, sdf, devn, col, ren = _build(R, "default_64x64", render=O.RenderConf(n_samples=32, n_importance=0))
    px, py = CU.surface_pixels(rig["kinv"][v], rig["pose"][v], rig["H"], rig["W"], B_STEP, seed=17)
    t_rand = torch.rand(B_STEP, 1, generator=torch.Generator().manual_seed(23))
    ref, s, out = _device_step(R, ren, rig, v, px, py, DELTA, LOG_SCALE, False, t_rand)
    assert s["near"].grad_fn is not None and out["color_fine"].grad_fn is not None
    rgb, mask = s["true_rgb"].detach().cpu(), s["mask"].detach().cpu()
    torch.set_num_threads(16)
    g64 = _oracle_step(p, mc, rig, mode, v, px, py, DELTA, LOG_SCALE, False, None, t_rand, rgb, mask, torch.float64)
    g32 = _oracle_step(p, mc, rig, mode, v, px, py, DELTA, LOG_SCALE, False, None, t_rand, rgb, mask, torch.float32)
    _check_step("n_importance0", ref, v, g64, g32)


def test_bf16_refuses_the_refined_step_before_any_launch(R, rigs):
    rig, v = rigs["source"], VIEW["source"]
    dr = rig["dr"]
    mc, p, sdf, devn, col, ren = _build(R, "default_64x64")
    ren.set_variant(bf16=True)
    px, py = CU.pixels(B_STEP, rig["H"], rig["W"], seed=3)
    dr.set_refinement(_refinement(R, v))
    try:
        s = dr.sample(v, B_STEP, pixels_x=px, pixels_y=py)
        ren.last_z_vals = None
        with pytest.raises(RuntimeError, match="bf16.*no input adjoints"):
            ren.render_rnb(s["rays_o"], s["rays_d"], s["near"], s["far"], s["lights_dir"])
        assert ren.last_z_vals is None, "the refusal must come before the sampling launches"
        with torch.no_grad():      # forward only, the refined camera renders in bf16 as any other
            q = dr.sample(v, B_STEP, pixels_x=px, pixels_y=py)
        out = ren.render_rnb(q["rays_o"], q["rays_d"], q["near"], q["far"], q["lights_dir"])
        assert bool(torch.isfinite(out["color_fine"]).all())
    finally:
        dr.set_refinement(None)
