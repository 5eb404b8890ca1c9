"""What the GPU test files share: the module-scoped `R` fixture, the device, the end-to-end step against the fp64 oracle
(the rule itself is tests/parity.py), the SURVEY 8c counts, the profiler's kernel classes.  Not a test module: test
modules import from here, never from each other (a test module imported as `tests.test_x` is a second copy of the one
pytest collected, with its own module-level state)."""
import ctypes as C
import json
import os
import socket

import pytest
import torch

from oracle import rnb_oracle as O
from tests import parity as P

FUSED_CLASSES = {"F_sweep(save)", "R_sweep", "FB_sweep", "RA_sweep", "dW(x3: 256x256 + narrow jobs)"}
ALBEDO_H2_CLASSES = {"albedo_fwd", "albedo_bwd"}


@pytest.fixture(scope="module")
def R():
    """the package with its native library loaded; a GPU test file gets it with `from tests.gpu_support import R`"""
    assert torch.cuda.is_available(), "GPU tests need a device"
    import rnb_neus_fork_amd as pkg
    pkg.native.load()
    torch.set_num_threads(16)
    return pkg


def device():
    return torch.device("cuda:0")


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def explicit_depths(batch, S, seed):
    """sorted non-uniform depths [B, S] between near and far, from the generator seed given"""
    gen = torch.Generator().manual_seed(seed)
    u = torch.sort(torch.rand(batch["near"].shape[0], S, generator=gen), dim=-1).values
    return (batch["near"] + (batch["far"] - batch["near"]) * u).contiguous()


def profile_classes(R):
    """the kernel classes the library's profiler has seen since rnb_profile_enable(1)"""
    lib = R.native.load()
    ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
    R.native.check(lib.rnb_profile_collect(C.byref(ms), C.byref(n), C.byref(fl)))
    need = lib.rnb_profile_report(None, 0)
    buf = C.create_string_buffer(int(need) + 16)
    lib.rnb_profile_report(buf, len(buf))
    return {ln.rsplit(" ", 3)[0] for ln in buf.value.decode().splitlines()}


def build_golden(R, g):
    """the device modules of a golden fixture: (named parameters, sdf, deviation, colour, renderer)"""
    p = g.params()
    sdf, dev, col, ren = R.build_from_named_params(g.mc, p, device())
    # development aid: RNB_TEST_NO_X2H=1 runs the golden suite on the six-bf16-term arithmetic (the SURVEYTOL lines of that run
    # are what DESIGN 2 compares the default's against; the recorded floor is NOT held in that mode)
    if os.environ.get("RNB_TEST_NO_X2H") and g.mc.sdf.d_hidden == 256:
        ren.set_variant(x2h=False)
    return p, sdf, dev, col, ren


def named(sdf, dev, col):
    out = {("sdf." + k): v for k, v in sdf.named_parameters()}
    out["dev.variance"] = dev.variance
    out.update({("color." + k): v for k, v in col.named_parameters()})
    return out


def assert_has_surface(out, dvariance=None):
    """Non-degeneracy guard: the rendered scene has a surface (otherwise weights, CDFs and colours are ~0 and every
    absolute bound passes for zeros) and the variance gradient is resolved."""
    assert float(out["weight_sum"].mean()) > 0.3, "degenerate scene: rays do not hit a surface"
    assert float(out["weights"].max()) > 1e-2, "degenerate scene: no sample carries weight"
    if dvariance is not None:
        assert float(dvariance.abs().max()) > 1e-6, "degenerate scene: d loss / d variance vanishes"


# SURVEY 8c states |d| <= 1e-5 + 1e-4 |ref| (outputs) and rel-L2 <= 1e-4 per gradient tensor.  The calibrated bounds of
# tests/parity.py replace them where the fp32 reference itself is further than that from fp64; how many tensors still meet
# the ORIGINAL bounds is counted, printed, and held to the floor measured on MI355X in round 4
# (tests/golden/survey_tol_floor.json: a drift towards the calibrated bounds' 3 x would otherwise pass unseen).
def survey_counts(got_all, ref32_all, grads_mine, grads_ref):
    n_out = ok_out = n_g = ok_g = 0
    missed = []
    for k, ref in ref32_all.items():
        if k == "inside_sphere":
            continue
        d = (got_all[k].double() - ref.double()).abs()
        n_out += 1
        ok = bool((d <= 1e-5 + 1e-4 * ref.double().abs()).all())
        ok_out += int(ok)
        if not ok:
            missed.append(f"{k} (max excess {float((d - 1e-5 - 1e-4 * ref.double().abs()).max()):.1e})")
    for k, ref in grads_ref.items():
        rn = float(ref.double().norm())
        if rn < 1e-10:
            continue
        n_g += 1
        rel = float((grads_mine[k].double() - ref.double()).norm()) / rn
        ok_g += int(rel <= 1e-4)
        if rel > 1e-4:
            missed.append(f"d {k} ({rel:.1e})")
    return ok_out, n_out, ok_g, n_g, missed


SURVEY_FLOOR_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "survey_tol_floor.json")
_SURVEY_SEEN = {}      # tag -> (outputs ok, gradient tensors ok) of this session: the ONE record the aggregate test reads


def check_survey(tag, counts):
    ok_out, n_out, ok_g, n_g, missed = counts
    _SURVEY_SEEN[tag] = (ok_out, ok_g)
    print(f"SURVEYTOL {tag}: outputs within 1e-5 + 1e-4|ref| of the fp32 reference: {ok_out}/{n_out}; "
          f"gradient tensors within rel-L2 1e-4: {ok_g}/{n_g}" + (f"; outside: {', '.join(missed)}" if missed else ""))
    # [r5] The default path has no floating-point atomics any more (every reduction is a fixed-order slab sum: DESIGN 2), so
    # these counts are deterministic: a build is held to the recorded ones EXACTLY — no slack per fixture, none in aggregate
    # (test_survey_tolerance_counts_in_aggregate).  The record is not regenerated by the change it judges: the 13 round-4
    # entries are round 4's, the three round-5 fixtures were added with their first measurement.
    floor = None
    if not os.environ.get("RNB_TEST_NO_X2H") and os.path.exists(SURVEY_FLOOR_PATH):
        floor = json.load(open(SURVEY_FLOOR_PATH)).get(tag)
    if floor is not None:
        assert ok_out >= floor["outputs_ok"], f"{tag}: {ok_out} outputs meet SURVEY 8c's bound, {floor['outputs_ok']} are on record"
        assert ok_g >= floor["grads_ok_measured"], \
            f"{tag}: {ok_g} gradient tensors meet SURVEY 8c's bound, {floor['grads_ok_measured']} are on record"


@torch.no_grad()
def device_sampling_trace(R, g, sdf, b, z0):
    """The up-sampling loop of rnb_sample_rays composed from the public per-step entry points (rnb_up_sample_step,
    rnb_sdf_forward, rnb_gather_sdf), so that the integer outputs of every step are visible.  (no_grad, like the reference's
    loop, models/renderer.py:590: the direct network calls raise under grad mode.)"""
    lib = R.native.load()
    d = device()
    rc = g.mc.render
    ro, rd = b["rays_o"].contiguous(), b["rays_d"].contiguous()
    B = ro.shape[0]
    n_new = rc.n_importance // rc.up_sample_steps
    z = z0.contiguous()
    pts = ro[:, None, :] + rd[:, None, :] * z[..., None]
    sdfv = sdf.sdf(pts.reshape(-1, 3)).reshape(B, -1).contiguous()
    inds_all = []
    for i in range(rc.up_sample_steps):
        n = z.shape[1]
        new_z = torch.empty(B, n_new, device=d)
        inds = torch.empty(B, n_new, dtype=torch.int32, device=d)
        z_out = torch.empty(B, n + n_new, device=d)
        sidx = torch.empty(B, n + n_new, dtype=torch.int32, device=d)
        R.native.check(lib.rnb_up_sample_step(R.native.ptr(ro), R.native.ptr(rd), R.native.ptr(z), R.native.ptr(sdfv),
                                              B, n, n_new, float(64 * 2 ** i), R.native.ptr(new_z), R.native.ptr(inds),
                                              R.native.ptr(z_out), R.native.ptr(sidx), None))
        inds_all.append(inds.cpu().long())
        if i + 1 < rc.up_sample_steps:
            npts = ro[:, None, :] + rd[:, None, :] * new_z[..., None]
            new_sdf = sdf.sdf(npts.reshape(-1, 3)).reshape(B, n_new).contiguous()
            merged = torch.empty(B, n + n_new, device=d)
            R.native.check(lib.rnb_gather_sdf(R.native.ptr(sdfv), R.native.ptr(new_sdf), R.native.ptr(sidx), B, n,
                                              n_new, R.native.ptr(merged), None))
            sdfv = merged
        z = z_out
    return inds_all, z


STEP_OUT_KEYS = ("color_fine", "weights", "weight_sum", "gradients", "cdf_fine", "gradient_error")


def step_against_fp64(R, mc, p, sdf, dev, col, ren, batch, tag, survey=True, z_vals=None, stats=None, loss_rule="fixed"):
    """One END-TO-END train-shaped step on the device (sampling + fine pass + loss + backward) against the CPU oracle in fp64
    on the z_vals the device sampled; outputs and every parameter gradient bounded by the fp32 oracle's own distance from fp64
    (tests/parity.py).  `p`: the named parameters (CPU tensors) the device modules were built from.  `z_vals` given: the
    step renders at those depths instead of sampling (the same fine pass and backward).  `stats`: a dict that receives the
    worst output and gradient error as fractions of their bounds and the number of gradient tensors checked.  `loss_rule`:
    "fixed" holds the loss to rtol 1e-5 / atol 1e-6 of the fp64 oracle's; "calibrated" (tests/test_gpu_ray_matrix.py) widens
    that to K_OUT x the fp32 oracle's own loss error where the fp32 oracle itself is outside the fixed tolerance — at 512
    samples per ray on a state whose rays saturate (weight_sum at the BCE's clip) the reference's fp32 arithmetic is 1.4e-5
    from fp64, on the same depths, and so is the device."""
    b = {k: v.to(device()) for k, v in batch.items()}
    if z_vals is None:
        out = ren.render_rnb(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=1.0,
                             t_rand=b["t_rand"])
    else:
        out = ren.render_rnb(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=1.0,
                             z_vals=z_vals.to(device()))
    loss = O.rnb_loss(out, b["true_rgb"], b["mask"])[0]
    loss.backward()
    torch.cuda.synchronize()
    assert_has_surface(out, dev.variance.grad)
    z = ren.last_z_vals.cpu()
    torch.set_num_threads(16)
    # ground truth in float64 (bias gradients are sums of 65,536 signed terms: an fp32 CPU sum is itself
    # only good to ~1e-3 there, so both fp32 implementations are measured against the fp64 oracle)
    pr = {k: v.detach().double().requires_grad_(True) for k, v in p.items()}
    b64 = {k: v.double() for k, v in batch.items()}
    ref = O.render_rnb(pr, mc, b64["rays_o"], b64["rays_d"], b64["near"], b64["far"], b64["lights_dir"],
                       cos_anneal_ratio=1.0, z_vals=z.double())
    ref_loss = O.rnb_loss(ref, b64["true_rgb"], b64["mask"])[0]
    ref_loss.backward()
    # the same step with the oracle in fp32 (the reference's own arithmetic) calibrates outputs and gradients
    p32 = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    ref32 = O.render_rnb(p32, mc, batch["rays_o"], batch["rays_d"], batch["near"], batch["far"],
                         batch["lights_dir"], cos_anneal_ratio=1.0, z_vals=z)
    O.rnb_loss(ref32, batch["true_rgb"], batch["mask"])[0].backward()
    worst_out = ("", 0.0)
    for k in STEP_OUT_KEYS:
        ratio = P.check_value(f"{tag}: {k}", out[k], ref[k].detach(), ref32[k].detach())
        if ratio > worst_out[1]:
            worst_out = (k, ratio)
    if loss_rule == "fixed":
        torch.testing.assert_close(loss.detach().cpu().double(), ref_loss.detach(), rtol=1e-5, atol=1e-6)
    else:
        assert loss_rule == "calibrated", loss_rule
        l64 = float(ref_loss)
        e_hip, e_ref = abs(float(loss) - l64), abs(float(O.rnb_loss(ref32, batch["true_rgb"], batch["mask"])[0]) - l64)
        bound = max(1e-6 + 1e-5 * abs(l64), P.ref_term(e_ref))     # never below the fixed tolerance
        print(f"{tag}: loss |hip - fp64| {e_hip:.3e}, fp32 oracle {e_ref:.3e}, bound {bound:.3e}")
        assert e_hip <= bound, f"{tag}: loss: |hip - fp64| {e_hip:.3e} > {bound:.3e} (fp32 CPU oracle: {e_ref:.3e})"
    params = named(sdf, dev, col)
    worst = ("", 0.0, 0.0)
    n_checked = 0
    for k, v in params.items():
        rg = pr[k].grad
        assert float(rg.norm()) > 1e-9, f"{k}: the fp64 gradient vanishes: not a parity target"
        assert bool(torch.isfinite(v.grad).all()), f"{tag}: gradient of {k} is not finite"
        rel32 = P.rel_l2(p32[k].grad, rg)
        assert rel32 <= P.GRAD_CAP / P.K_GRAD, f"{k}: the fp32 oracle itself is {rel32:.2e} from fp64: not a parity target"
        mine = v.grad.cpu()
        ratio = P.check_grad(f"{tag}: {k}", mine, rg, rel32)
        if ratio > worst[1]:
            worst = (k, ratio, P.rel_l2(mine, rg))
        n_checked += 1
    print(f"{tag} vs fp64 oracle: weight_sum mean {float(out['weight_sum'].mean()):.3f}; worst output {worst_out[0]}: "
          f"{worst_out[1]:.2f} of its bound; worst gradient {worst[0]}: rel-L2 {worst[2]:.2e} = {worst[1]:.2f} of its bound")
    if stats is not None:
        stats.update(worst_out=worst_out, worst_grad=worst[:2], n_checked=n_checked)
    if survey:
        # SURVEY 8c's original bounds, against the fp32 oracle (the reference's arithmetic) on the same depths
        check_survey(tag, survey_counts({k: out[k].detach().cpu() for k in STEP_OUT_KEYS},
                                        {k: ref32[k].detach() for k in STEP_OUT_KEYS},
                                        {k: v.grad.cpu() for k, v in params.items()}, {k: p32[k].grad for k in params}))
    return out
