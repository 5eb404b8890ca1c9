"""The per-ray kernels ("one wave64 per ray") over the table of tests/ray_matrix.py, on the device.

sampling.hip (z_init_kernel, up_sample_kernel, gather_sdf_kernel), composite.hip (fine_points_kernel, composite_fwd_kernel,
composite_bwd_body, ray_input_adjoint_kernel) and the fused loss read their sizes at run time and walk a ray in 64-lane
pieces with a carry between pieces.  Every row of the table runs here:
  1. up_sample_kernel alone (rnb_up_sample_step) on every (n, n_new) of the table: the merge exactly, the searchsorted
     indices exactly outside measured near ties, the new depths by the calibrated output rule against the fp64 oracle;
  2. rows built to take the kernel's serial fallback;
  3. one train step per accepted row (device sampling, fine pass, loss, backward; every parameter gradient against fp64) on
     the per-layer path (w32) and, for six rows, on the fused sweeps (default_64x64);
  4. rnb_sample_rays against the loop composed from the per-step entry points, bit for bit, and the initial depths against
     the oracle's, bit for bit (odd n);
  5. explicit z_vals at S = 1 .. 512 through render, render_rnb and render_rnb_warmup against fp64;
  6. every refused row: RuntimeError, and the library's profiler lists no kernel class (refused before a launch);
  7. three rows on RNB_VARIANT_BF16 against oracle/bf16_emu.py.
The input gradients with explicit depths (z_vals.grad, light counts) are in tests/test_gpu_render_input_grads.py.
Every accepted row prints one line starting with RAYROW."""
import contextlib
from dataclasses import replace
from types import SimpleNamespace

import pytest
import torch

from oracle import rnb_oracle as O
from tests import parity as P
from tests import ray_matrix as M
from tests.bf16_emu_step import step as bf16_step
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import ALBEDO_H2_CLASSES, FUSED_CLASSES, assert_has_surface, device, device_sampling_trace, \
    explicit_depths, profile_classes, step_against_fp64
from tests.shape_matrix import BY_NAME as SHAPE_BY_NAME, live_params, step_batch

pytestmark = pytest.mark.gpu

W32 = SHAPE_BY_NAME["w32"]
FUSED = SHAPE_BY_NAME["default_64x64"]
SENTINEL_I = -7


def _build(R, shape, row):
    mc = replace(shape.mc, render=row.render_conf)
    p = live_params(mc, shape.seed)
    sdf, dev, col, ren = R.build_from_named_params(mc, p, device())
    return mc, p, sdf, dev, col, ren


@contextlib.contextmanager
def _fp64_default():
    """the oracle's sampling functions create their constants (linspace, zeros) in the default dtype"""
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------------------------- 1
def _run_up_sample_step(R, ref, n_new, inv_s):
    """rnb_up_sample_step on the reference's inputs; every output pre-filled with a sentinel"""
    lib = R.native.load()
    d = device()
    z_in, sdf_in = ref["z"].to(d), ref["sdf"].to(d)
    ro, rd = ref["rays_o"].to(d), ref["rays_d"].to(d)
    B, n = z_in.shape
    new_z = torch.full((B, n_new), float("nan"), device=d)
    inds = torch.full((B, n_new), SENTINEL_I, dtype=torch.int32, device=d)
    z_out = torch.full((B, n + n_new), float("nan"), device=d)
    sidx = torch.full((B, n + n_new), SENTINEL_I, dtype=torch.int32, device=d)
    R.native.check(lib.rnb_up_sample_step(R.native.ptr(ro), R.native.ptr(rd), R.native.ptr(z_in), R.native.ptr(sdf_in), B, n,
                                          n_new, float(inv_s), R.native.ptr(new_z), R.native.ptr(inds), R.native.ptr(z_out),
                                          R.native.ptr(sidx), None))
    torch.cuda.synchronize()
    return new_z.cpu(), inds.cpu().long(), z_out.cpu(), sidx.cpu().long()


def _check_up_sample_case(R, n, n_new, inv_s, tag):
    """one (n, n_new, inv_s): returns (samples, exempt, flipped among the exempt, new_z error as a fraction of its bound)"""
    ref = M.up_sample_reference(n, n_new, inv_s)
    new_z, inds, z_out, sidx = _run_up_sample_step(R, ref, n_new, inv_s)
    B = new_z.shape[0]
    # the merge: exactly the stable sort of what the device merged, every slot written
    assert bool(torch.isfinite(new_z).all()), f"{tag}: new_z has unwritten (NaN pre-fill) or non-finite slots"
    assert bool(torch.isfinite(z_out).all()), f"{tag}: z_out has unwritten slots"
    assert int(inds.min()) >= 0 and int(inds.max()) <= n, f"{tag}: inds outside [0, n] (or the sentinel)"
    cat = torch.cat([ref["z"], new_z], -1)
    want = torch.sort(cat, dim=1, stable=True)
    assert torch.equal(sidx, want.indices), f"{tag}: sort_index is not the stable sort of cat[z_in, new_z]"
    assert torch.equal(z_out, torch.gather(cat, 1, sidx)), f"{tag}: z_out is not the depths gathered by sort_index"
    assert torch.equal(torch.sort(sidx, dim=1).values, torch.arange(n + n_new).expand(B, -1)), f"{tag}: not a permutation"
    # the indices: exact, except where a cdf value lies within the measured margin of its u
    cdf2 = M.up_sample_cdf_reexpressed(ref["rays_o"], ref["rays_d"], ref["z"], ref["sdf"], inv_s)
    exempt, margin = M.near_tie_exempt(ref["cdf"], cdf2, n_new)
    k = int(exempt.sum())
    assert k <= max(1.0, 1e-3 * exempt.numel()), f"{tag}: {k} near ties of {exempt.numel()} samples: a bad input, not a pass"
    diff = inds != ref["inds"]
    flipped_exempt = int((diff & exempt).sum())
    print(f"UPSAMPLE {tag}: margin {margin:.2e}, exempt {k}/{exempt.numel()}, flipped among them {flipped_exempt}, "
          f"flipped outside {int((diff & ~exempt).sum())}")
    assert not bool((diff & ~exempt).any()), \
        f"{tag}: {int((diff & ~exempt).sum())} searchsorted indices differ from the oracle's away from any near tie"
    # the new depths: the output rule against the fp64 oracle
    with _fp64_default():
        o64 = O.up_sample(ref["rays_o"].double(), ref["rays_d"].double(), ref["z"].double(), ref["sdf"].double(), n_new, inv_s)
    e_hip, e_ref, bound = P.value_errors(new_z, o64, ref["new_z"])
    print(f"UPSAMPLE {tag}: new_z |hip - fp64| {e_hip:.3e}, fp32 oracle {e_ref:.3e}, bound {bound:.3e}")
    return exempt.numel(), k, flipped_exempt, P.check_value(f"{tag}: new_z", new_z, o64, ref["new_z"])


_UP_TOTALS = {"samples": 0, "exempt": 0}


@pytest.mark.parametrize("pair", M.up_sample_pairs(), ids=[f"{n}_{k}" for n, k in M.up_sample_pairs()])
def test_up_sample_kernel(R, pair):
    n, n_new = pair
    for inv_s in M.UP_INV_S:
        tot, k, _, _ = _check_up_sample_case(R, n, n_new, inv_s, f"n={n} n_new={n_new} inv_s={inv_s:g}")
        _UP_TOTALS["samples"] += tot
        _UP_TOTALS["exempt"] += k


def test_up_sample_kernel_near_ties_in_aggregate(R):
    """over all cases together at most 0.02 % of the samples may be exempt (the host test counts the same on the CPU)"""
    if _UP_TOTALS["samples"] == 0:      # run on its own: count here
        for n, n_new in M.up_sample_pairs():
            for inv_s in M.UP_INV_S:
                ref = M.up_sample_reference(n, n_new, inv_s)
                cdf2 = M.up_sample_cdf_reexpressed(ref["rays_o"], ref["rays_d"], ref["z"], ref["sdf"], inv_s)
                exempt, _ = M.near_tie_exempt(ref["cdf"], cdf2, n_new)
                _UP_TOTALS["samples"] += exempt.numel()
                _UP_TOTALS["exempt"] += int(exempt.sum())
    print(f"UPSAMPLE all cases: {_UP_TOTALS['exempt']} exempt of {_UP_TOTALS['samples']} samples")
    assert _UP_TOTALS["exempt"] <= 2e-4 * _UP_TOTALS["samples"]


# ------------------------------------------------------------------------------------------------------------------- 2
FALLBACK_INV_S = -4.0


@pytest.mark.parametrize("pair", [(66, 7), (129, 13), (448, 64)], ids=lambda p: f"{p[0]}_{p[1]}")
def test_up_sample_serial_cdf_fallback(R, pair):
    """Rows that must take up_sample_kernel's serial CDF scan (`wj >= 7.45e-9 && wj < 4` fails), with the properties of
    test_up_sample_kernel.

    With sorted depths and inv_s > 0 that test cannot fail on finite data: alpha lies in (0, 1], so every raw weight is
    alpha T + 1e-5 >= 1e-5 while the weights telescope to a sum <= 1 + 512e-5, i.e. every pdf value is >= 9.9e-6, far above
    2^-27.  What reaches the fallback through the public entry point is a caller's inv_s < 0 (a plain float argument of
    rnb_up_sample_step): next_cdf > prev_cdf makes alpha negative, the raw weights change sign, and a pdf value below
    2^-27 of the sum (here: below zero) sends the whole ray to the sequential scan.  The oracle's arithmetic is defined for
    it (torch.cumsum keeps its running value in double, as the serial scan does); asserted below on the CPU, per ray,
    before the device runs.  (A NaN row takes the same branch: tests/test_gpu_parity.py
    test_nan_rays_poison_only_themselves.)

    The other fallback — a transmittance whose double running product lies within 2e-13 relative of an fp32 rounding
    boundary (scan_safe) — is NOT constructed here.  Whether the device's running product is that close to a boundary
    depends on the last bits of every alpha, and those come from the device's expf, which is not bit-identical to
    torch.exp (the reason the indices above are exact only outside near ties); a row found on the CPU with the oracle's
    double product would sit about 1e-8 relative away from where the device's product sits, five orders of magnitude more
    than the window.  Rows with saturated sigmoids (alpha bit-identical on both sides) give only the products c^k d^m of
    two constants: a few 1e4 distinct values against a hit rate of 4e-6 per value."""
    n, n_new = pair
    ref = M.up_sample_reference(n, n_new, FALLBACK_INV_S)
    pdf = ref["cdf"][:, 1:] - ref["cdf"][:, :-1]
    takes_fallback = (~((pdf >= 7.450580596923828e-09) & (pdf < 4.0))).any(dim=1)
    assert bool((pdf < -1e-6).any(dim=1).all()) and bool(takes_fallback.all()), "every ray must fail the kernel's pdf test"
    assert bool(torch.isfinite(ref["new_z"]).all())
    tot, k, fl, frac = _check_up_sample_case(R, n, n_new, FALLBACK_INV_S, f"fallback n={n} n_new={n_new} inv_s={FALLBACK_INV_S:g}")
    print(f"UPSAMPLE fallback n={n} n_new={n_new}: {int(takes_fallback.sum())}/{len(takes_fallback)} rays through the serial "
          f"scan; exempt {k}/{tot}, new_z at {frac:.2f} of its bound")


# ------------------------------------------------------------------------------------------------------------------- 3
def _batch(row, B, step=1):
    """the rays of tests/shape_matrix.py step_batch (seed 11, step 1), with the row's light count"""
    return O.synthetic_batch(B, n_lights=row.n_lights, seed=11, step=step, warmup=False)


def _row_step(R, shape, row, B, batch_step=1):
    lib = R.native.load()
    mc, p, sdf, dev, col, ren = _build(R, shape, row)
    stats = {}
    tag = f"{row.name} {shape.name}"
    lib.rnb_profile_enable(1)
    try:
        out = step_against_fp64(R, mc, p, sdf, dev, col, ren, _batch(row, B, batch_step), tag, survey=False, stats=stats,
                                 loss_rule="calibrated")
        classes = profile_classes(R)
    finally:
        lib.rnb_profile_enable(0)
    assert tuple(ren.last_z_vals.shape) == (B, row.S)
    assert tuple(out["color_fine"].shape) == (row.n_lights, B, 3)
    assert stats["n_checked"] == len(O.param_order(mc))
    print(f"RAYROW {row.name} step [{shape.name}: {shape.path}] S={row.S} n_new={row.n_new} lights={row.n_lights}: classes "
          f"{sorted(classes)}; worst output {stats['worst_out'][0]} {stats['worst_out'][1]:.2f}, worst gradient "
          f"{stats['worst_grad'][0]} {stats['worst_grad'][1]:.2f} of its bound")
    return classes


@pytest.mark.parametrize("row", M.ACCEPTED, ids=[r.name for r in M.ACCEPTED])
def test_train_step_per_layer_path(R, row):
    """16 rays on w32 (per-layer GEMMs, cheap fp64): B * S is a multiple of 64 only where S is a multiple of 4"""
    classes = _row_step(R, W32, row, 16)
    assert "layer_gemm" in classes and not ((FUSED_CLASSES | ALBEDO_H2_CLASSES) & classes)


FUSED_ROWS = [M.BY_NAME[n] for n in M.FUSED_ROW_NAMES]
# The rays of a fused row: step_batch's (seed 11, step 1) unless the row is listed here.  64+448/7 takes step 2: on step 1's
# rays ONE ReLU decision of the albedo network's second layer (one point, unit 110) falls on the other side of zero than
# in the fp64 oracle, in the default arithmetic and on the per-layer route alike (not with six bf16 terms, not in the fp32
# oracle).  The gradient of color.lin1.bias is then wrong in that one unit by 1.34e-6 (all other units together: 7.3e-8, i.e.
# 4e-6 relative) and every gradient of the albedo network reads 0.8 - 1.08e-4 from fp64 against a bound of 1e-4 (fp32 oracle:
# 2e-5).  A pre-activation within rounding of a kink is no parity target for any fp32 arithmetic; with 64 x 512 points x 512
# ReLUs about one per step is expected.  On the rays of steps 2, 3 and 4 the row reads 0.31, 0.32, 0.31 of its bound.  The
# same rays give 65+64/1 its 0.79 (unit 51, 1.03e-6 of 1.034e-6); it stays on them, inside its bound.
FUSED_BATCH_STEP = {"64+448/7": 2}


@pytest.mark.parametrize("row", FUSED_ROWS, ids=[r.name for r in FUSED_ROWS])
def test_train_step_fused_sweeps(R, row):
    """64 rays on the shipped shape (with 16 its state renders weight_sum 0.28, below assert_has_surface's 0.3)"""
    classes = _row_step(R, FUSED, row, 64, FUSED_BATCH_STEP.get(row.name, 1))
    assert FUSED_CLASSES <= classes and ALBEDO_H2_CLASSES <= classes, sorted(classes)


@pytest.mark.parametrize("B", [16, 32])
def test_train_step_fused_sweeps_with_one_split_per_weight_gradient_job(R, B):
    """2+0 at 16 and 32 rays: 32 and 64 points, where every job of the one-workgroup weight-gradient kernel has a single
    split and the slab workspace holds exactly one slab of each.  (Found by the z_vals.grad case at S = 2: the room clamp's
    equal-share rule computed a share of zero for a 256-column job followed by 64-column ones and refused the backward
    with "weight-gradient slab workspace exhausted".)  This state renders a surface at both sizes (weight_sum 0.49, 0.47)."""
    classes = _row_step(R, FUSED, M.BY_NAME["2+0"], B)
    assert FUSED_CLASSES <= classes and ALBEDO_H2_CLASSES <= classes, sorted(classes)


# ------------------------------------------------------------------------------------------------------------------- 4
SAMPLING_ROWS = [r for r in M.BASE_ROWS]


@pytest.mark.parametrize("shape", [W32, FUSED], ids=lambda s: s.name)
@pytest.mark.parametrize("row", SAMPLING_ROWS, ids=[r.name for r in SAMPLING_ROWS])
def test_sampling_equals_the_composed_loop(R, shape, row):
    """rnb_sample_rays == rnb_up_sample_step + rnb_sdf_forward + rnb_gather_sdf composed over the row's steps, bit for bit;
    the initial depths == the oracle's (torch.linspace's two halves at odd n), bit for bit"""
    B = 48
    mc, p, sdf, dev, col, ren = _build(R, shape, row)
    batch = step_batch(B)
    b = {k: v.to(device()) for k, v in batch.items()}
    packed = ren._pack(False)
    z = ren.sample_z_vals(b["rays_o"], b["rays_d"], b["near"], b["far"], packed, 1.0, b["t_rand"])
    ren0 = R.NeuSRenderer(None, sdf, dev, col, n_samples=row.n_samples, n_importance=0, n_outside=0, up_sample_steps=1,
                          perturb=1.0)
    z0 = ren0.sample_z_vals(b["rays_o"], b["rays_d"], b["near"], b["far"], packed, 1.0, b["t_rand"])
    torch.cuda.synchronize()
    mc0 = replace(mc, render=O.RenderConf(n_samples=row.n_samples, n_importance=0))
    z0_ref = O.sample_rays(p, mc0, batch["rays_o"], batch["rays_d"], batch["near"], batch["far"], batch["t_rand"], 1.0)
    assert tuple(z.shape) == (B, row.S)
    assert torch.equal(z0.cpu(), z0_ref), f"{row.name}: the initial depths differ from torch.linspace's (n = {row.n_samples})"
    assert bool((z[:, 1:] >= z[:, :-1]).all()), "depths must be sorted"
    assert bool(torch.isfinite(z).all())
    if row.n_importance == 0:
        assert torch.equal(z, z0)
        print(f"RAYROW {row.name} sampling [{shape.name}]: initial depths bit-exact (no importance samples)")
        return
    inds_all, z_composed = device_sampling_trace(R, SimpleNamespace(mc=mc), sdf, b, z0)
    assert [tuple(i.shape) for i in inds_all] == [(B, row.n_new)] * row.up_sample_steps
    for i, n in zip(inds_all, row.step_n):
        assert int(i.min()) >= 0 and int(i.max()) <= n
    assert torch.equal(z_composed, z), f"{row.name}: rnb_sample_rays differs from the loop composed from the per-step entry points"
    # against the oracle's own loop: not bit-exact (the loop amplifies last-bit differences of the SDF), reported only
    zo = O.sample_rays(p, mc, batch["rays_o"], batch["rays_d"], batch["near"], batch["far"], batch["t_rand"], 1.0)
    close = float(((z.cpu() - zo).abs() < 1e-4).float().mean())
    print(f"RAYROW {row.name} sampling [{shape.name}]: z0 bit-exact, composed loop bit-exact over {row.up_sample_steps} steps; "
          f"depths within 1e-4 of the oracle's loop: {close:.4f}")


def test_initial_depths_on_the_unit_interval_are_torch_linspace(R):
    """z_init_kernel with near = 0, far = 1 and no perturbation returns linspace_at(0, 1, n, j) itself: equal to
    torch.linspace(0, 1, n) bit for bit for every n from 2 to 512.  Through a ray's own near / far the last bit of the middle
    element is usually rounded away again (z0 of the rows above stays bit-exact with linspace_at's split moved to
    (steps + 1) / 2); here that split changes a value at 79 odd n, 127 and 191 of the table among them
    (tests/test_ray_matrix_host.py restates both splits on the CPU)."""
    mc, p, sdf, dev, col, ren = _build(R, W32, M.BY_NAME["2+0"])
    packed = ren._pack(False)
    b = {k: v.to(device()) for k, v in step_batch(2).items()}
    near, far = torch.zeros(2, 1, device=device()), torch.ones(2, 1, device=device())
    wrong = []
    for n in range(2, M.K_MAX_S + 1):
        r = R.NeuSRenderer(None, sdf, dev, col, n_samples=n, n_importance=0, n_outside=0, up_sample_steps=1, perturb=0.0)
        z = r.sample_z_vals(b["rays_o"], b["rays_d"], near, far, packed, 0.0)
        if not torch.equal(z.cpu(), torch.linspace(0.0, 1.0, n).expand(2, n)):
            wrong.append(n)
    assert not wrong, f"initial depths differ from torch.linspace(0, 1, n) at n = {wrong[:20]} ({len(wrong)} values of n)"


# ------------------------------------------------------------------------------------------------------------------- 5
def _oracle_render(p, mc, api, batch, z, bg, dt):
    q = {k: v.to(dt) for k, v in p.items()}
    x = {k: v.to(dt) for k, v in batch.items()}
    if api == "render":
        out = O.render(q, mc, x["rays_o"], x["rays_d"], x["near"], x["far"], background_rgb=bg.to(dt), cos_anneal_ratio=0.5,
                       z_vals=z.to(dt))
    else:
        out = O.render_rnb(q, mc, x["rays_o"], x["rays_d"], x["near"], x["far"], x["lights_dir"], cos_anneal_ratio=0.5,
                           warmup=api == "render_rnb_warmup", z_vals=z.to(dt))
    return {k: v.detach() for k, v in out.items()}


@pytest.mark.parametrize("shape", [W32, FUSED], ids=lambda s: s.name)
@pytest.mark.parametrize("S", M.Z_VALS_S)
def test_explicit_depths_forward_against_fp64(R, shape, S):
    """render, render_rnb and render_rnb_warmup, forward only, at S explicit depths: every float output (weight_max
    included) by the output rule.  S = 1, 2: less than a chunk; 65 .. 511: a carry into a ragged chunk; 512 = kMaxS."""
    B = 16
    mc = shape.mc
    p = live_params(mc, shape.seed)
    sdf, dev, col, ren = R.build_from_named_params(mc, p, device())
    batch = step_batch(B)
    z = explicit_depths(batch, S, seed=104729 + S)
    b = {k: v.to(device()) for k, v in batch.items()}
    bg = torch.tensor([0.2, 0.5, 0.8])
    worst = ("", 0.0)
    for api in ("render", "render_rnb", "render_rnb_warmup"):
        with torch.no_grad():
            if api == "render":
                out = ren.render(b["rays_o"], b["rays_d"], b["near"], b["far"], background_rgb=bg.to(device()),
                                 cos_anneal_ratio=0.5, z_vals=z.to(device()))
            else:
                fn = ren.render_rnb_warmup if api == "render_rnb_warmup" else ren.render_rnb
                out = fn(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=0.5,
                         z_vals=z.to(device()))
        torch.cuda.synchronize()
        r64 = _oracle_render(p, mc, api, batch, z, bg, torch.float64)
        r32 = _oracle_render(p, mc, api, batch, z, bg, torch.float32)
        if S >= 63:
            assert_has_surface(r64)
        assert torch.equal(out["inside_sphere"].cpu(), r32["inside_sphere"].reshape(B, S))
        for k in M.FLOAT_OUTS:
            ratio = P.check_value(f"S={S} {shape.name} {api} {k}", out[k], r64[k].reshape(out[k].shape),
                                  r32[k].reshape(out[k].shape))
            if ratio > worst[1]:
                worst = (f"{api} {k}", ratio)
    print(f"RAYROW z{S} explicit depths [{shape.name}]: worst output {worst[0]} {worst[1]:.2f} of its bound")


# ------------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("shape", [W32, FUSED], ids=lambda s: s.name)
@pytest.mark.parametrize("row", M.REFUSED, ids=[f"{r.name}:{r.limit}" for r in M.REFUSED])
def test_refused_rows_are_refused_before_any_launch(R, shape, row):
    """Argument checks, not experiments: a sampling row is refused by rnb_sample_workspace_bytes (the renderer asks it before
    rnb_sample_rays, which runs check_sampling_desc itself before its first launch); S = 513 by rnb_render_workspace_bytes
    (asked before rnb_render_fwd, whose render_setup repeats the check before carve_render); 9 lights by render_setup.
    Before either, the renderer has only packed the weights (rnb_weightnorm_fwd: indexed by the network shape, not by S or
    the light count).  The profiler, which tags every sweep, GEMM and weight-gradient launch, must list no kernel class."""
    lib = R.native.load()
    B = 16
    mc, p, sdf, dev, col, ren = _build(R, shape, row)
    batch = O.synthetic_batch(B, n_lights=row.n_lights, seed=11, step=1, warmup=False)
    b = {k: v.to(device()) for k, v in batch.items()}
    # (the 9-light row renders at explicit depths too: its own sampling would be a legitimate launch before the refusal)
    S = row.z_vals_S or 32
    z = None if row.refused_by == "sample_query" else explicit_depths(batch, S, seed=104729 + S).to(device())
    ren.last_z_vals = None
    for api in ("render_rnb", "render"):
        lib.rnb_profile_enable(1)
        try:
            with pytest.raises(RuntimeError, match=row.limit):
                if api == "render":
                    ren.render(b["rays_o"], b["rays_d"], b["near"], b["far"], t_rand=b["t_rand"], z_vals=z)
                else:
                    ren.render_rnb(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], t_rand=b["t_rand"], z_vals=z)
            torch.cuda.synchronize()
            classes = profile_classes(R)
        finally:
            lib.rnb_profile_enable(0)
        assert classes == set(), f"{row.name} {api}: kernels ran before the refusal: {sorted(classes)}"
        if row.refused_by == "call":
            break      # (render has no lights: the 9-light row is a render_rnb call)
    if row.refused_by == "sample_query":
        assert ren.last_z_vals is None, "refused before the sampling"
    print(f"RAYROW {row.name} refused [{shape.name}]: {row.refused_by}, message names {row.limit!r}, no kernel class launched")


# ------------------------------------------------------------------------------------------------------------------- 7
BF16_ROWS = [M.BY_NAME[n] for n in M.BF16_ROW_NAMES]


@pytest.mark.parametrize("row", BF16_ROWS, ids=[r.name for r in BF16_ROWS])
def test_bf16_step_against_emulation(R, row):
    """RNB_VARIANT_BF16 shares sampling.hip and composite.hip with the fp32 variants; its point buffers are its own.
    48 rays, as that file's 256-sample steps.  (Measured with 16 rays: 129+39/3 inside every bound; 65+64/1 and 64+448/7
    outside for the last SDF layer alone — sdf.lin8.weight_g 2.4e-2 and 3.1e-2 from the fp64 emulation against bounds of
    1.5e-2 and 8.1e-3, the emulation's own fp32 orders 8.8e-3 and 2.0e-3 — the most cancelling gradient of the network over
    2,064 and 8,192 points.)"""
    mc = O.ModelConf(render=row.render_conf)
    n = bf16_step(R, mc, 48, tag=f"RAYROW {row.name} bf16 S={row.S}")
    assert n >= 25
