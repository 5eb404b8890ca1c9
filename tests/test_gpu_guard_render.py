"""Train-shaped steps through NeuSRenderer between guard bands (tests/guard_bands.py): no kernel of a render, its sampling or
its backward may store outside the buffers the call was given, and nothing read from outside them may reach a result.

The rule every case follows: the step (render, loss, backward) runs once on ordinary allocations and once under
guarded() with its inputs passed through guard(); then both bands of every allocation must still hold their pattern, the
registry must have seen the buffers the call is known to make (a workspace of exactly rnb_render_workspace_bytes, the
sampling workspace, the packed weights and packed_grad, the flat gradient buffer, every output and input-gradient shape), and
every output, depth, extra and gradient must equal the unguarded run bit for bit.  The bodies of torch.empty buffers hold the
bands' pattern as well: this is also test_uninitialised_workspace_is_never_read on every shape.  No fp64 oracle.  The loss is
O.rnb_loss plus a fixed random linear functional of every float output, so that no output adjoint is NULL.

Not reproducible between two runs of their own (fp32 atomics in a weight-gradient or bias reduction), and therefore held to
"finite exactly where the unguarded run is finite" in their GRADIENTS (outputs, depths and extras are bit-equal everywhere):
reproducible() below names them: RNB_VARIANT_BF16 without DETERMINISTIC, every shape on the per-layer path and every fused
shape whose albedo network runs as layer GEMMs, the variants generic, dw_lds, dw_staged, f32_mfma and x2h=False, and the
default route at a point count that is no multiple of 32 (its weight gradients then leave the split-K kernels).  Everything
else, and everything under RNB_VARIANT_DETERMINISTIC, is bit-equal.

The last test is the detector's own positive control on the device: one output of a render is handed out 4 bytes short.
Every case prints one line starting with GUARD (guarded allocations, wall time)."""
import ctypes as C
import time
from dataclasses import replace

import pytest
import torch

from oracle import rnb_oracle as O
from tests import guard_bands as GB
from tests import point_matrix as PM
from tests import ray_matrix as M
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device, explicit_depths, named
from tests.shape_matrix import BY_NAME, SHAPES, STEP_RENDER, live_params
from tests.variant_matrix import VARIANTS

pytestmark = pytest.mark.gpu

RENDER_SHAPES = [s for s in SHAPES if s.render]
DEFAULT = BY_NAME["default_64x64"]
W32 = BY_NAME["w32"]
BF16_DET = dict(bf16=True, deterministic=True)


def reproducible(shape, variant, M):
    """False: two unguarded runs of this shape under this variant over M points give different gradient bits, because a
    weight-gradient or bias reduction of theirs leaves through fp32 atomics (measured on the MI355X: profiles/guard_bands_gpu.txt)"""
    v = dict(variant)
    if v.get("deterministic"):
        return True                        # every reduction through ordered slabs
    if v.get("bf16"):
        return False                       # bf16_dw.hip, bf16_color.hip
    if not shape.fused or v.get("generic"):
        return False                       # the per-layer path: layers.hip, dw.hip.h
    if not shape.color_h2:
        return False                       # fused SDF sweeps, the albedo network as layer GEMMs
    if v.get("dw_lds") or v.get("dw_staged") or v.get("f32_mfma") or v.get("x2h") is False:
        return False                       # the other weight-gradient kernels and arithmetics
    return PM.runs_x3(M)                   # the default route: slabs over whole 32-point chunks, split-K atomics otherwise


@pytest.fixture(autouse=True)
def _release():
    yield
    GB.release()                           # the registry keeps every guarded allocation alive until here


def _functional(out, seed=5):
    """a fixed random linear functional of every float output (O(1) per tensor), as tests/test_gpu_render_input_grads.py"""
    g = torch.Generator().manual_seed(seed)
    total = 0.0
    for k in M.FLOAT_OUTS:
        t = out[k]
        w = torch.randn(tuple(t.shape), generator=g, dtype=torch.float64) / max(1, t.numel()) ** 0.5
        total = total + (w.to(t.device, t.dtype) * t).sum()
    return total


def _flags(R, api, no_albedo, per_ray_lights, forward_only, input_grads):
    n = R.native
    f = {"render": n.MODE_CORE, "rnb": n.MODE_MVPS, "warmup": n.MODE_MVPS | n.FLAG_RELU_SHADING}[api]
    if api != "render":
        f |= (n.FLAG_NO_ALBEDO if no_albedo else 0) | (n.FLAG_LIGHT_PER_RAY if per_ray_lights else 0)
    return f | (n.FLAG_FORWARD_ONLY if forward_only else 0) | (n.FLAG_INPUT_GRADS if input_grads else 0)


def _run(R, ren, sdf, devn, col, batch, g, api="rnb", want=(), z_vals=None, bg=None, no_albedo=False, no_grad=False):
    """one step; `g`: what every input passes through (identity, or guard_bands.guard).  Returns everything comparable."""
    for q in list(sdf.parameters()) + list(devn.parameters()) + list(col.parameters()):
        q.grad = None
    ren._range = None
    b = dict(batch)
    if z_vals is not None:
        b["z_vals"] = z_vals
    if bg is not None:
        b["bg"] = bg
    x = {k: g(v.to(device())).requires_grad_(k in want) for k, v in b.items()}
    kw = dict(cos_anneal_ratio=0.5, t_rand=x["t_rand"], z_vals=x.get("z_vals"))
    with torch.set_grad_enabled(not no_grad):
        if api == "render":
            out = ren.render(x["rays_o"], x["rays_d"], x["near"], x["far"], background_rgb=x.get("bg"), **kw)
        else:
            fn = ren.render_rnb if api == "rnb" else ren.render_rnb_warmup
            out = fn(x["rays_o"], x["rays_d"], x["near"], x["far"], x["lights_dir"], no_albedo=no_albedo, **kw)
        true_rgb = x["true_rgb"] if api != "render" else x["true_rgb"][:1]
        loss = _functional(out) + O.rnb_loss(out, true_rgb, x["mask"])[0]
        if not no_grad:
            loss.backward()
    torch.cuda.synchronize()
    res = dict(out={k: v.detach() for k, v in out.items()}, z=ren.last_z_vals, loss=loss.detach(),
               extras=dict(ren.last_extras))
    if ren.track_range:
        res["range"] = ren._range.clone()
    grads = {}
    if not no_grad:
        grads = {k: v.grad for k, v in named(sdf, devn, col).items() if v.grad is not None}
        grads.update({"input." + k: x[k].grad for k in want})
        assert all(x[k].grad is not None for k in want)
    return res, grads


def _case(R, tag, shape, mc, B, variant=None, batch=None, n_lights=3, warmup_lights=False, repro=None, short=None, **call):
    """the rule of the module docstring on one step; returns the guarded session"""
    t0 = time.perf_counter()
    variant = dict(variant or {})
    p = live_params(mc, shape.seed)
    sdf, devn, col, ren = R.build_from_named_params(mc, p, device())
    ren.set_variant(**variant)
    for k in ("want_extras", "track_range"):
        setattr(ren, k, bool(call.pop(k, False)))
    if batch is None:
        batch = O.synthetic_batch(B, n_lights=n_lights, seed=11, step=1, warmup=warmup_lights)
    clean, clean_grads = _run(R, ren, sdf, devn, col, batch, lambda t: t, **call)
    with GB.guarded(shortchange=short) as s:
        got, got_grads = _run(R, ren, sdf, devn, col, batch, GB.guard, **call)
        if short is not None:
            return s, s.damaged()
        s.assert_intact(tag)
    # ---- positive controls: the registry saw what the call is known to allocate
    api, want, no_grad = call.get("api", "rnb"), call.get("want", ()), call.get("no_grad", False)
    S = got["z"].shape[1]
    lib, nbytes = R.native.load(), C.c_int64()
    per_ray = api != "render" and batch["lights_dir"].numel() != batch["lights_dir"].shape[0] * 3
    flags = _flags(R, api, call.get("no_albedo", False), per_ray, no_grad, bool(want))
    R.native.check(lib.rnb_render_workspace_bytes(C.byref(ren.desc), B, S, flags, C.byref(nbytes)))
    assert s.seen(nbytes=nbytes.value, dtype=torch.uint8), \
        f"{tag}: no guarded buffer of rnb_render_workspace_bytes = {nbytes.value}: " \
        f"{[e.describe() for e in s.seen(dtype=torch.uint8)]}"
    if call.get("z_vals") is None:
        R.native.check(lib.rnb_sample_workspace_bytes(C.byref(ren.desc), B, C.byref(nbytes)))
        assert s.seen(nbytes=max(nbytes.value, 256), dtype=torch.uint8), f"{tag}: the sampling workspace was not guarded"
    n_packed = R.runtime.packed_floats(ren.desc)
    assert len(s.seen(shape=(n_packed,), dtype=torch.float32)) >= (1 if no_grad else 2), \
        f"{tag}: packed weights{'' if no_grad else ' and packed_grad'} were not guarded"
    for k, v in got["out"].items():
        assert s.seen(shape=tuple(v.shape), dtype=torch.float32), f"{tag}: output {k} {tuple(v.shape)} was not guarded"
    for k, v in got["extras"].items():
        assert s.seen(shape=tuple(v.shape), dtype=torch.float32), f"{tag}: extra {k} was not guarded"
    if not no_grad:
        use_color = not (api != "render" and call.get("no_albedo", False))
        total = sum(q.numel() for q in ren._leaves(use_color))
        assert s.seen(shape=(total,), dtype=torch.float32), f"{tag}: the flat gradient buffer [{total}] was not guarded"
    for k in want:      # the gradient buffer has the shape the library sees: [L, B, 1, 3] lights are [L, B, 3] there
        native_shape = tuple(d for d in got_grads["input." + k].shape if d != 1)
        assert [e for e in s.seen(shape=native_shape, dtype=torch.float32) if "backward" in e.site], \
            f"{tag}: the gradient buffer of {k} {native_shape} was not guarded"
    # ---- the same bits
    GB.assert_same(tag, clean, got)
    rep = reproducible(shape, variant, B * S) if repro is None else repro
    try:
        GB.assert_same(tag + " gradients", clean_grads, got_grads, reproducible=rep)
    except AssertionError as e:
        if not rep:
            raise
        again, again_grads = _run(R, ren, sdf, devn, col, batch, lambda t: t, **call)
        try:
            GB.assert_same(tag, clean_grads, again_grads)
        except AssertionError as e2:
            raise AssertionError(f"{e}\n  (two UNGUARDED runs differ as well: {e2}: this case is not reproducible)") from None
        raise AssertionError(f"{e}\n  (two unguarded runs agree bit for bit: the guarded run is what differs)") from None
    if not rep:         # (printed, not asserted: atomics may well agree on one pair of runs)
        _, again_grads = _run(R, ren, sdf, devn, col, batch, lambda t: t, **call)
        differ = [k for k in clean_grads if not GB.same_bits(clean_grads[k], again_grads[k])]
        print(f"GUARD render {tag}: two unguarded runs differ in {len(differ)} of {len(clean_grads)} gradient tensors")
    print(f"GUARD render {tag}: {len(s.registry)} guarded allocations, {'bit-equal' if rep else 'finite-where-finite'} gradients, "
          f"{time.perf_counter() - t0:.2f} s")
    return s, []


# ------------------------------------------------------------------------------------------------------------------- 1
def _shape_cases():
    out = []
    for s in RENDER_SHAPES:
        out.append(pytest.param(s, {}, id=s.name))
        if s.bf16:
            out.append(pytest.param(s, BF16_DET, id=s.name + "-bf16_det"))
    return out


# make_layout accepts 15 hidden layers on the bf16 route, its backward does not: they are more weight-gradient jobs than one
# bf16 launch holds (bf16_dw.hip kMaxBfDwJobs), and bf16_dw_backward refuses the launch with RNB_E_INVALID: a loud error, held
BF16_REFUSED = {"nl15": "too many weight-gradient jobs"}


@pytest.mark.parametrize("shape,variant", _shape_cases())
def test_every_shape_at_37_rays(R, shape, variant):
    """37 rays x 32 samples = 1184 points: pad_rows adds 96 rows to every point-tiled buffer"""
    if variant and shape.name in BF16_REFUSED:
        with pytest.raises(R.native.NativeError, match=BF16_REFUSED[shape.name]):
            _case(R, f"{shape.name} bf16", shape, replace(shape.mc, render=STEP_RENDER), 37, variant)
        return
    _case(R, f"{shape.name} {variant or 'default'}", shape, replace(shape.mc, render=STEP_RENDER), 37, variant)


# ------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_every_variant_on_the_shipped_shape(R, variant):
    _case(R, f"default_64x64 {variant[0]}", DEFAULT, DEFAULT.mc, 37, variant[1])


# ------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("row", M.ACCEPTED, ids=[r.name for r in M.ACCEPTED])
def test_every_ray_row_on_the_per_layer_path(R, row):
    """5 rays: B * S is a multiple of 64 only where S is"""
    _case(R, f"w32 {row.name}", W32, replace(W32.mc, render=row.render_conf), 5, n_lights=row.n_lights)


FUSED_ROWS = [M.BY_NAME[n] for n in M.FUSED_ROW_NAMES]
BF16_ROWS = [M.BY_NAME[n] for n in M.BF16_ROW_NAMES]


@pytest.mark.parametrize("row", FUSED_ROWS, ids=[r.name for r in FUSED_ROWS])
def test_ray_rows_on_the_fused_sweeps(R, row):
    _case(R, f"default_64x64 {row.name}", DEFAULT, replace(DEFAULT.mc, render=row.render_conf), 5, n_lights=row.n_lights)


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("row", BF16_ROWS, ids=[r.name for r in BF16_ROWS])
def test_ray_rows_on_the_bf16_route(R, row, det):
    _case(R, f"default_64x64 bf16{' deterministic' if det else ''} {row.name}", DEFAULT,
          replace(DEFAULT.mc, render=row.render_conf), 5, dict(bf16=True, deterministic=det), n_lights=row.n_lights)


# ------------------------------------------------------------------------------------------------------------------- 4
def test_render_with_a_background(R):
    _case(R, "render + background", DEFAULT, DEFAULT.mc, 37, api="render", bg=torch.tensor([0.2, 0.5, 0.8]))


@pytest.mark.parametrize("no_albedo", [True, False], ids=["no_albedo", "albedo"])
def test_render_rnb_warmup(R, no_albedo):
    _case(R, f"warmup no_albedo={no_albedo}", DEFAULT, DEFAULT.mc, 37, api="warmup", no_albedo=no_albedo, warmup_lights=True)


@pytest.mark.parametrize("L", [1, 8])
def test_per_ray_lights(R, L):
    s, _ = _case(R, f"per-ray lights L={L}", DEFAULT, DEFAULT.mc, 37, n_lights=L)
    assert s.seen(shape=(L, 37, 3), dtype=torch.float32)


@pytest.mark.parametrize("S", [2, 65, 512])
def test_explicit_depths(R, S):
    batch = O.synthetic_batch(37, seed=11, step=1)
    _case(R, f"z_vals S={S}", DEFAULT, DEFAULT.mc, 37, batch=batch, z_vals=explicit_depths(batch, S, seed=S))


def test_forward_only_under_no_grad(R):
    _case(R, "no_grad", DEFAULT, DEFAULT.mc, 37, no_grad=True)


def test_want_extras(R):
    s, _ = _case(R, "want_extras", DEFAULT, DEFAULT.mc, 37, want_extras=True)
    assert s.seen(shape=(37 * 128, 1)) and s.seen(shape=(37, 128, 3))


@pytest.mark.parametrize("no_grad", [False, True], ids=["train", "forward_only"])
def test_track_range(R, no_grad):
    s, _ = _case(R, f"track_range no_grad={no_grad}", DEFAULT, DEFAULT.mc, 37, track_range=True, no_grad=no_grad)
    assert s.seen(shape=(8,), dtype=torch.float32)


# ------------------------------------------------------------------------------------------------------------------- 5
INPUT_GRAD_CASES = [("rays", "rnb", ("rays_o", "rays_d")), ("lights", "rnb", ("lights_dir",)),
                    ("shared_lights", "warmup", ("lights_dir",)), ("background", "render", ("bg",)),
                    ("z_vals", "rnb", ("z_vals",)), ("all_rnb", "rnb", ("rays_o", "rays_d", "lights_dir", "z_vals")),
                    ("all_render", "render", ("rays_o", "rays_d", "bg", "z_vals"))]


@pytest.mark.parametrize("case", INPUT_GRAD_CASES, ids=[c[0] for c in INPUT_GRAD_CASES])
def test_input_gradient_backward(R, case):
    """rnb_render_bwd_inputs with each of rays, lights, background and z_vals requiring grad, alone and together"""
    name, api, want = case
    batch = O.synthetic_batch(37, seed=11, step=1, warmup=api == "warmup")
    z = explicit_depths(batch, 65, seed=3) if "z_vals" in want else None
    bg = torch.tensor([0.2, 0.5, 0.8]) if api == "render" else None
    _case(R, f"input grads {name}", DEFAULT, DEFAULT.mc, 37, batch=batch, api=api, want=want, z_vals=z, bg=bg)


# ------------------------------------------------------------------------------------------------------------------- 6
FULL = replace(DEFAULT, name="full_size", mc=O.ModelConf())


@pytest.mark.parametrize("B", [1, 3, 129, 200])
@pytest.mark.parametrize("variant", [{}, BF16_DET], ids=["default", "bf16_det"])
def test_ray_counts_on_the_full_size_network(R, B, variant):
    """128 samples per ray: 1, 3 and 129 rays end inside a padded tile, 200 x 128 is the one count with no padded row"""
    _case(R, f"full size B={B} {variant or 'default'}", FULL, FULL.mc, B, variant)


# ------------------------------------------------------------------------------------------------------------------- 7
def test_the_bands_are_live_on_the_device(R):
    """`weights` [37, 128] is handed out with a body 4 bytes shorter than asked (same allocation, same view): the composite's
    store of the last ray's last weight then lands in the first 4 bytes of what is now the trailing band - memory this test
    owns - and damaged() must name that buffer, that band and offset 0.  Nothing else may be reported."""
    B, S = 37, 128
    batch = O.synthetic_batch(B, seed=11, step=1)
    # explicit depths: with sampling the first [B, S] allocation of the step would be sample_z_vals' own
    s, hurt = _case(R, "shortchanged weights", DEFAULT, DEFAULT.mc, B, batch=batch, z_vals=explicit_depths(batch, S, seed=1),
                    short=((B, S), 4))
    assert len(hurt) == 1, hurt
    d = hurt[0]
    assert d["band"] == "trailing" and d["shape"] == (B, S) and d["dtype"] == torch.float32, d
    assert d["nbytes"] == B * S * 4 - 4 and d["first"] - d["nbytes"] == 0 and d["last"] - d["nbytes"] <= 3, d
    assert "forward" in d["site"], d
    with pytest.raises(AssertionError, match="trailing band"):
        s.assert_intact("shortchanged weights")
