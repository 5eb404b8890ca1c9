"""rnb_render_maps / NeuSRenderer.render_maps on the device: the per-ray maps of a forward-only render.

  1. colour and weight_sum are the existing wrappers' bits (same launches up to the composite, same expressions in it);
  2. normal, albedo and depth against the float64 sums of the existing forward's own per-sample outputs, at a bound derived
     from the kernel's arithmetic, over S = 1 .. 512, 1 / 3 / 8 lights (shared and per ray, with and without the warm-up's
     ReLU) and B = 1, 65 — with a guard that the inside-sphere mask matters in every case;
  3. every golden fixture against the reference's fp32 / fp64 outputs by the calibrated rule of tests/parity.py;
  4. refusals before any launch, and grad mode;
  5. the workspace is one chunk's, whatever the number of rays.
"""
import ctypes as C
import math

import pytest
import torch

from oracle import rnb_oracle as O
from tests import parity as P
from tests.golden_util import Golden, case_names
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device, profile_classes

pytestmark = pytest.mark.gpu

CASES = case_names()
BIT_CASES = ["tiny_main_sharp", "tiny_warmup_sharp", "tiny_render_bg", "tiny_main_noalbedo", "full_main_sharp"]
RNB_E_INVALID = -1


def _build(R, g):
    p = g.params()
    sdf, dev, col, ren = R.build_from_named_params(g.mc, p, device())
    return p, sdf, dev, col, ren


def _wrapper(ren, api, b, z, cos, no_albedo=False, bg=None):
    """the existing forward under no_grad (forward-only), with its optional per-sample extras"""
    ren.want_extras = True
    try:
        with torch.no_grad():
            kw = dict(cos_anneal_ratio=cos, z_vals=z)
            if api == "render":
                out = ren.render(b["rays_o"], b["rays_d"], b["near"], b["far"], background_rgb=bg, **kw)
            else:
                fn = ren.render_rnb_warmup if api == "render_rnb_warmup" else ren.render_rnb
                out = fn(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], no_albedo=no_albedo, **kw)
        out = dict(out)
        out.update(ren.last_extras)
    finally:
        ren.want_extras = False
    return out


def _maps(ren, api, b, z, cos, no_albedo=False, bg=None, **kw):
    return ren.render_maps(b["rays_o"], b["rays_d"], b["near"], b["far"], b.get("lights_dir"), api=api, z_vals=z,
                           cos_anneal_ratio=cos, no_albedo=no_albedo, background_rgb=bg, **kw)


def _golden_pair(R, name, variant=None, **kw):
    g = Golden(name)
    p, sdf, dev, col, ren = _build(R, g)
    if variant:
        ren.set_variant(**variant)
    b = {k: v.to(device()) for k, v in g.batch.items()}
    z = g.z_fine.to(device())
    bg = b.get("background_rgb")
    ref = _wrapper(ren, g.api, b, z, g.cos_anneal_ratio, g.no_albedo, bg)
    got = _maps(ren, g.api, b, z, g.cos_anneal_ratio, g.no_albedo, bg, **kw)
    torch.cuda.synchronize()
    return g, p, ref, got


# ------------------------------------------------------------------------------------------------------------------- 1
BIT_PARAMS = [(n, None) for n in BIT_CASES] + [("full_main_sharp", dict(bf16=True)), ("full_main_sharp", dict(f32_mfma=True))]


@pytest.mark.parametrize("name,variant", BIT_PARAMS,
                         ids=[n + ("" if v is None else "-" + "-".join(v)) for n, v in BIT_PARAMS])
def test_colour_and_weight_sum_are_the_wrappers_bits(R, name, variant):
    g, p, ref, got = _golden_pair(R, name, variant, maps=("color", "weight_sum", "weight_max", "normal", "depth"))
    assert float(ref["weight_sum"].mean()) > 0.3, "degenerate scene"
    assert got["color"].shape == ref["color_fine"].shape and got["weight_sum"].shape == ref["weight_sum"].shape
    assert torch.equal(got["color"], ref["color_fine"]), f"{name}: colour differs from the wrapper's bits"
    assert torch.equal(got["weight_sum"], ref["weight_sum"])
    assert torch.equal(got["weight_max"], ref["weight_max"])
    # asking for fewer maps does not change the bits of the rest
    only = _maps(*_rebuild_args(R, name, variant), maps=("color",))
    assert torch.equal(only["color"], ref["color_fine"]) and set(only) == {"color"}


def _rebuild_args(R, name, variant):
    g = Golden(name)
    p, sdf, dev, col, ren = _build(R, g)
    if variant:
        ren.set_variant(**variant)
    b = {k: v.to(device()) for k, v in g.batch.items()}
    return ren, g.api, b, g.z_fine.to(device()), g.cos_anneal_ratio, g.no_albedo, b.get("background_rgb")


# ------------------------------------------------------------------------------------------------------------------- 2
MATRIX_S = [1, 63, 64, 65, 130, 512]     # less than a chunk, one lane idle, a full chunk, a carry + 1, + a ragged one, kMaxS
MATRIX_B = [1, 65]
MATRIX_L = [1, 3, 8]
_MATRIX_RAYS = {}


def matrix_rays():
    """65 rays of O.synthetic_batch ordered by decreasing distance of the ray from the origin: ray 0 (the B = 1 case)
    passes 0.8 from it, so about half its depth range lies outside the unit sphere."""
    if not _MATRIX_RAYS:
        b = O.synthetic_batch(65, seed=11, step=1, warmup=False)
        closest = b["rays_o"] + b["rays_d"] * (-(b["rays_o"] * b["rays_d"]).sum(-1, keepdim=True))
        order = torch.argsort(closest.norm(dim=-1), descending=True)
        _MATRIX_RAYS.update({k: b[k][order].contiguous() for k in ("rays_o", "rays_d", "near", "far")})
    return _MATRIX_RAYS


def matrix_depths(S, B):
    """sorted random depths in (near, far); with S = 1 every other ray's only sample sits at a tenth of the range, outside
    the unit sphere for the rays that pass far from the origin (ray 0 among them)"""
    r = matrix_rays()
    gen = torch.Generator().manual_seed(7919 + S)
    u = torch.sort(0.03 + 0.94 * torch.rand(65, S, generator=gen), dim=-1).values
    if S == 1:
        u[::2, 0] = 0.1
    return (r["near"] + (r["far"] - r["near"]) * u)[:B].contiguous()


def matrix_lights(L, per_ray, B):
    gen = torch.Generator().manual_seed(31 * L + int(per_ray))
    t = torch.randn(L, 65 if per_ray else 1, 1, 3, generator=gen)
    t = t / t.norm(dim=-1, keepdim=True)
    return (t[:, :B] if per_ray else t).contiguous()


def reduction_bound(S, terms):
    """(ceil(S / 64) + 8) 2^-24 sum_s |term_s| per component.  One rounding per product at most (w * {0, 1} is exact and
    the products enter a fused multiply-add unrounded; the fp32 mid = z + dists / 2 is the expected value's own operand),
    ceil(S / 64) sequential fused adds per lane, six tree levels of the butterfly: every one of those roundings is
    relative to a partial sum that is at most sum |term|, and 1 + ceil(S / 64) + 6 <= ceil(S / 64) + 8."""
    return (math.ceil(S / 64) + 8) * 2.0 ** -24 * terms.abs().sum(dim=1)


def expected_maps(ref, z, n_samples):
    """float64 sums of the existing forward's own per-sample outputs"""
    w = ref["weights"].double().cpu()
    n = ref["gradients"].double().cpu()
    ins = ref["inside_sphere"].double().cpu()
    zc = z.cpu()
    dists = torch.cat([zc[:, 1:] - zc[:, :-1], torch.full_like(zc[:, :1], 2.0 / n_samples)], -1)
    mid = (zc + dists * 0.5).double()                  # fp32 mid, as fine_points_kernel forms it
    terms = {"normal": w[..., None] * n * ins[..., None], "normal_nomask": w[..., None] * n, "depth": (w * mid)[..., None]}
    if "sampled_albedo" in ref:
        terms["albedo"] = w[..., None] * ref["sampled_albedo"].double().cpu().reshape(w.shape[0], w.shape[1], -1)
    return terms


def _check_reductions(got, terms, S, tag):
    worst = 0.0
    for k in ("normal", "albedo", "depth"):
        if k not in terms:
            continue
        want = terms[k].sum(dim=1)
        bound = reduction_bound(S, terms[k])
        err = (got[k].double().cpu().reshape(want.shape) - want).abs()
        print(f"MAPS {tag} {k}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}")
        assert bool((err <= bound).all()), f"{tag} {k}: {float((err - bound).max()):.3e} over the bound"
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    return worst


@pytest.mark.parametrize("B", MATRIX_B)
@pytest.mark.parametrize("S", MATRIX_S)
def test_reductions_against_the_per_sample_outputs(R, S, B):
    g = Golden("tiny_main_sharp")
    p, sdf, dev, col, ren = _build(R, g)
    rays = {k: v[:B].to(device()) for k, v in matrix_rays().items()}
    z = matrix_depths(S, B).to(device())
    ns = g.mc.render.n_samples
    first = True
    for L in MATRIX_L:
        for per_ray in (False, True):
            for api in ("render_rnb", "render_rnb_warmup"):
                b = dict(rays, lights_dir=matrix_lights(L, per_ray, B).to(device()))
                ref = _wrapper(ren, api, b, z, 0.5)
                got = _maps(ren, api, b, z, 0.5, maps=("color", "normal", "albedo", "depth", "weight_sum", "weight_max"))
                tag = f"S={S} B={B} L={L} {'per-ray' if per_ray else 'shared'} {api}"
                assert got["color"].shape == (L, B, 3)
                assert torch.equal(got["color"], ref["color_fine"]), f"{tag}: colour"
                assert torch.equal(got["weight_sum"], ref["weight_sum"]) and torch.equal(got["weight_max"], ref["weight_max"])
                terms = expected_maps(ref, z, ns)
                if first:      # (the per-sample outputs do not depend on the lights)
                    first = False
                    assert float(ref["weights"].sum()) > 0.0 and bool(torch.isfinite(got["normal"]).all())
                    # guard: without the mask the expected normal is another number, by more than the bound
                    gap = (terms["normal_nomask"].sum(dim=1) - terms["normal"].sum(dim=1)).abs()
                    assert bool((gap > reduction_bound(S, terms["normal"])).any()), f"{tag}: the mask is not tested"
                    outside = 1.0 - float(ref["inside_sphere"].mean())
                    print(f"MAPS {tag}: {100 * outside:.0f} % of the samples outside the sphere, largest gap "
                          f"{float(gap.max()):.3e}")
                    _check_reductions(got, terms, S, tag)
                else:
                    for k in ("normal", "albedo", "depth"):
                        want = terms[k].sum(dim=1)
                        err = (got[k].double().cpu().reshape(want.shape) - want).abs()
                        assert bool((err <= reduction_bound(S, terms[k])).all()), f"{tag} {k}"


# ------------------------------------------------------------------------------------------------------------------- 3
def _rule(got, ref32, ref64, what):
    got = got.reshape(ref64.shape)
    e_hip, e_ref, bound = P.value_errors(got, ref64, ref32)
    print(f"MAPS {what}: |hip - fp64| {e_hip:.3e}, fp32 reference {e_ref:.3e}, bound {bound:.3e}")
    P.check_value(what, got, ref64, ref32)


def _mid(z, n_samples):
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 2.0 / n_samples)], -1)
    return z + dists * 0.5


@pytest.mark.parametrize("name", CASES)
def test_maps_against_the_reference(R, name):
    g = Golden(name)
    with_albedo = g.api != "render" and not g.no_albedo
    maps = ("color", "normal", "depth", "weight_sum", "weight_max") + (("albedo",) if with_albedo else ())
    g, p, ref, got = _golden_pair(R, name, maps=maps)
    o32, o64 = g.out, g.out64
    ins = o32["inside_sphere"]
    n32 = (o32["gradients"] * o32["weights"][:, :, None] * ins[..., None]).sum(dim=1)          # exp_runner.py:466-469
    n64 = (o64["gradients"] * o64["weights"][:, :, None] * ins.double()[..., None]).sum(dim=1)
    assert float(n64.abs().max()) > 0.1, "degenerate scene: no normal map"
    _rule(got["color"], o32["color_fine"], o64["color_fine"], f"{name} color")
    _rule(got["weight_sum"], o32["weight_sum"], o64["weight_sum"], f"{name} weight_sum")
    _rule(got["weight_max"], o32["weight_max"], o64["weight_max"], f"{name} weight_max")
    _rule(got["normal"], n32, n64, f"{name} normal")
    ns = g.mc.render.n_samples
    d32 = (o32["weights"] * _mid(g.z_fine, ns)).sum(dim=1, keepdim=True)
    d64 = (o64["weights"] * _mid(g.z_fine.double(), ns)).sum(dim=1, keepdim=True)
    _rule(got["depth"], d32, d64, f"{name} depth")
    if with_albedo:
        res = {}
        for dt in (torch.float32, torch.float64):
            q = {k: v.to(dt) for k, v in p.items()}
            x = {k: v.to(dt) for k, v in g.batch.items()}
            r = O.render_rnb(q, g.mc, x["rays_o"], x["rays_d"], x["near"], x["far"], x["lights_dir"],
                             cos_anneal_ratio=g.cos_anneal_ratio, warmup=g.api == "render_rnb_warmup",
                             z_vals=g.z_fine.to(dt))
            res[dt] = (r["sampled_albedo"].detach() * r["weights"].detach()[:, :, None]).sum(dim=1)
        _rule(got["albedo"], res[torch.float32], res[torch.float64], f"{name} albedo")


# ------------------------------------------------------------------------------------------------------------------- 4
def _raw_call(R, ren, b, z, flags, n_lights, maps_ptrs, lights=None):
    """rnb_render_maps through ctypes; returns (code, message)"""
    lib = R.native.load()
    B, S = z.shape
    packed = ren._pack(True)
    nbytes = C.c_int64()
    R.native.check(lib.rnb_render_workspace_bytes(C.byref(ren.desc), B, min(S, 512), R.native.FLAG_FORWARD_ONLY | (flags & 7),
                                                  C.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=device())
    var = ren.deviation_network.variance.detach().reshape(1)
    a = R.native.RenderArgs()
    a.B, a.S, a.n_lights, a.flags, a.cos_anneal_ratio = B, S, n_lights, flags, 0.5
    a.rays_o, a.rays_d, a.z_vals, a.variance = b["rays_o"].data_ptr(), b["rays_d"].data_ptr(), z.data_ptr(), var.data_ptr()
    a.lights_dir = lights.data_ptr() if lights is not None else None
    m = R.native.RenderMapsOut()
    for k, t in maps_ptrs.items():
        setattr(m, k, t.data_ptr())
    with R.native.on_device(device()) as stream:
        rc = lib.rnb_render_maps(C.byref(ren.desc), R.native.ptr(packed), C.byref(a), C.byref(m), R.native.ptr(ws),
                                 ws.numel(), stream)
    return rc, lib.rnb_last_error_string().decode()


def test_refusals_come_before_any_launch(R):
    g = Golden("tiny_main_sharp")
    p, sdf, dev, col, ren = _build(R, g)
    N = R.native
    B = 4
    rays = {k: v[:B].to(device()) for k, v in matrix_rays().items()}
    z = matrix_depths(64, B).to(device())
    z513 = torch.sort(torch.rand(B, 513), dim=-1).values.to(device())
    l3 = matrix_lights(3, False, B).reshape(3, 3).to(device())
    l9 = matrix_lights(9, False, B).reshape(9, 3).to(device())
    f32 = dict(dtype=torch.float32, device=device())
    col3, alb, wsum = torch.empty(3, B, 3, **f32), torch.empty(B, 3, **f32), torch.empty(B, **f32)
    lib = N.load()
    lib.rnb_profile_enable(1)
    try:
        raw = [
            ("albedo in RNB_MODE_CORE", z, N.MODE_CORE, 1, dict(albedo=alb), None, "albedo"),
            ("albedo with RNB_FLAG_NO_ALBEDO", z, N.MODE_MVPS | N.FLAG_NO_ALBEDO, 3, dict(albedo=alb), l3, "albedo"),
            ("no map", z, N.MODE_MVPS, 3, dict(), l3, "no map"),
            ("S = 513", z513, N.MODE_MVPS, 3, dict(color=torch.empty(3, B, 3, **f32)), l3, "kMaxS"),
            ("9 lights", z, N.MODE_MVPS, 9, dict(color=torch.empty(9, B, 3, **f32)), l9, "kMaxRenderLights"),
            ("INPUT_GRADS", z, N.MODE_MVPS | N.FLAG_INPUT_GRADS, 3, dict(color=col3), l3, "INPUT_GRADS"),
        ]
        for what, zz, flags, nl, ptrs, lights, word in raw:
            rc, msg = _raw_call(R, ren, rays, zz, flags, nl, ptrs, lights)
            assert rc == RNB_E_INVALID, f"{what}: returned {rc} ({msg})"
            assert word in msg, f"{what}: the message does not name the limit: {msg!r}"
        # the Python entry point: an exception that names the limit
        b3 = dict(rays, lights_dir=l3.reshape(3, 1, 1, 3))
        with pytest.raises(ValueError, match="albedo"):
            _maps(ren, "render", rays, z, 0.5, maps=("color", "albedo"))
        with pytest.raises(ValueError, match="albedo"):
            _maps(ren, "render_rnb", b3, z, 0.5, no_albedo=True, maps=("albedo",))
        with pytest.raises(ValueError, match="maps"):
            _maps(ren, "render_rnb", b3, z, 0.5, maps=())
        with pytest.raises(RuntimeError, match="kMaxS"):
            _maps(ren, "render_rnb", b3, z513, 0.5)
        with pytest.raises(ValueError, match="kMaxRenderLights"):
            _maps(ren, "render_rnb", dict(rays, lights_dir=l9.reshape(9, 1, 1, 3)), z, 0.5)
        torch.cuda.synchronize()
        classes = profile_classes(R)
    finally:
        lib.rnb_profile_enable(0)
    assert classes == set(), f"kernels ran before a refusal: {sorted(classes)}"
    # (and the default map set of a mode without an albedo map simply leaves it out)
    out = _maps(ren, "render", rays, z, 0.5)
    assert set(out) == {"color", "normal", "depth", "weight_sum"} and out["color"].shape == (B, 3)


def test_no_graph_under_enable_grad(R):
    g = Golden("tiny_main_sharp")
    p, sdf, dev, col, ren = _build(R, g)
    leaves = list(sdf.parameters()) + list(col.parameters()) + [dev.variance]
    assert all(t.requires_grad for t in leaves)
    b = {k: v.to(device()) for k, v in g.batch.items()}
    b["rays_o"] = b["rays_o"].clone().requires_grad_(True)
    with torch.enable_grad():
        out = _maps(ren, g.api, b, g.z_fine.to(device()), g.cos_anneal_ratio, return_z_vals=True)
        assert torch.is_grad_enabled(), "the caller's grad mode is restored"
    assert set(out) == {"color", "normal", "albedo", "depth", "weight_sum", "z_vals"}
    for k, v in out.items():
        assert not v.requires_grad and v.grad_fn is None, k
    assert all(t.grad is None for t in leaves) and b["rays_o"].grad is None
    assert torch.equal(out["z_vals"], g.z_fine.to(device()))


# ------------------------------------------------------------------------------------------------------------------- 5
def test_workspace_is_one_chunks_whatever_the_ray_count(R):
    g = Golden("tiny_main_sharp")
    p, sdf, dev, col, ren = _build(R, g)
    S, L = 32, 3
    gen = torch.Generator().manual_seed(5)
    src = matrix_rays()
    idx = torch.randint(0, 65, (256,), generator=gen)
    rays = {k: v[idx].to(device()) for k, v in src.items()}
    lights = matrix_lights(L, False, 1).to(device())

    def peak_rise(n):
        r = {k: v[:n].contiguous() for k, v in rays.items()}
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = ren.render_maps(r["rays_o"], r["rays_d"], r["near"], r["far"], lights, api="render_rnb", perturb_overwrite=0,
                              cos_anneal_ratio=1.0, chunk_rays=64, maps=("color", "normal", "albedo", "depth", "weight_sum"))
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
        return rise, out

    peak_rise(64)                         # (warm the allocator and the weight cache)
    small, _ = peak_rise(64)
    large, out = peak_rise(256)
    assert out["normal"].shape == (256, 3) and bool(torch.isfinite(out["normal"]).all())
    # what 192 more rays may add: their slices of the inputs (o, d, near, far: 8 floats) and their rows of the outputs
    # (colour 3 L, normal 3, albedo 3, depth 1, weight_sum 1), each rounded up to the allocator's 512-byte granule
    extra = 192 * 4 * (8 + 3 * L + 3 + 3 + 1 + 1) + 16 * 512
    print(f"MAPS memory: peak rise {small} B at 64 rays, {large} B at 256 rays (chunk 64); allowed extra {extra + (1 << 20)} B")
    assert small > 0
    assert large - small <= extra + (1 << 20), f"the workspace grows with the image: {small} -> {large} bytes"
