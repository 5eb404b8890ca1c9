"""Input gradients of a render (rnb_render_bwd_inputs: rays_o, rays_d, z_vals, lights_dir, background_rgb) under each
cotangent of the render alone, against the fp64 oracle with the graph-keeping normal, over the table of
tests/input_adjoint_matrix.py (the rows of tests/adjoint_matrix.py and twelve more, no_albedo among them).

Every other device-vs-fp64 comparison of an input gradient drives all outputs and the training loss together; the paths by
which color_fine, weight_sum and gradient_error reach z_vals (ig_dists in composite_bwd_body<true>, the Dbar / carry_D stencil
and the Hessian term of ray_input_adjoint_kernel) carry 1e-3 of that combined gradient and are invisible to it.  Here

1. the table: each row renders at the table's depths with every input of its api requiring grad, takes the backward of
   sum(cotangent . out[adjoint]) and holds every input the adjoint reaches to the gradient rule of tests/parity.py per WHOLE
   tensor (never per ray: on rays that miss the surface, 1e-8 of the tensor, the fp32 oracle itself is 100 % off), every
   input it cannot reach — and under weight_max the rows of the rays the selection drops — to a finite, exact 0.0, the row's
   outputs to the output rule and the kernel classes to the shape's path.  One line INADJROW per (row, input).
2. variants: three rows under every fused_reverse_kernel instantiation reachable from set_variant (bwd_ti, bwd_nw, f32_mfma,
   x3, x2h=False), deterministic and generic — the R sweep stores ge only with input gradients — by the same rule and
   oracle; the arithmetic variants must also be seen to arrive (layer_gemm for generic, a gradient that differs in bits
   from the default's otherwise).
3. subsets: each input alone and two pairs, bit-equal to the call that wants every input; the parameter gradients bit-equal
   to the call that wants none.  Lights alone / background alone skip the point-wise adjoint (need_pbar false, ig given).
4. the no-albedo branch with per-ray and with shared lights.

What the rows see, measured with one-line arithmetic mutations of composite.hip (which table rows turn red; whether any test
of tests/test_gpu_render_input_grads.py does):
  the sign of ig_dists: z_vals red in every row whose adjoint passes alpha (color_fine, weights, cdf_fine, weight_sum,
    weight_max, all; both shapes, every api, both light shapes of case 4): rel-L2 1.3 .. 2.0, and 13 .. 22 under color_fine
    and weight_sum, where ig_dists and the mbar stencil nearly cancel.  The gradients and gradient_error rows stay green:
    their adjoint does not pass alpha, ig_dists is exactly zero under them.  Existing file: every test with z_vals or
    near / far red (0.1 .. 2.0), test_input_gradients_against_fp64 (no depth gradient) green.
  cos_d not added to d_bar: rays_d red in the same rows (1e-3 under cdf_fine .. 1.8e-2); gradients and gradient_error green
    (tcbar is zero under them).  Existing file: every fp64 comparison red (5e-3 .. 4e-2).
  pe_adjoint_hess(..., hess=false, ...): rays_o red in every row except s_val: 0.96 / 0.99 under gradients / gradient_error
    and 1e-2 (cdf_fine) .. 0.8 under the others on default_64x64, 3e-4 (cdf_fine) .. 8e-2 on w32.  Existing file: every
    fp64 comparison red (0.4 .. 1.0).
  0.5f * mb dropped from Db: z_vals red in every row except s_val (gradients 1.0, gradient_error 0.44, color_fine and
    weight_sum 3.1 .. 4.0, weights 0.07).  Existing file: the tests with z_vals or near / far red, the others green.
  nt[d] += gn[d] dropped: rays_o red under color_fine and all of render, render_rnb and render_rnb_warmup on default_64x64
    (3.7e-3 / 1.2e-3 under color_fine of render / render_rnb: 37 x / 12 x the bound; 4.8e-4 / 1.8e-4 under all) and, on w32,
    under color_fine of render (rays_o 4.1e-4) and of render_rnb_warmup (z_vals 7.0e-4 against 6.5e-4);
    w32-render_rnb-color_fine stays at 0.48 of its bound (rays_o 4.8e-5) and every no_albedo row green, as it must: with
    cinb == nullptr the term does not exist.  Existing file: red, but at
    1.1 .. 2.1 x the bound only (1.09e-4 against 1e-4 with one light): the combined functional sees this term at the edge
    of its floor, the color_fine rows see it an order of magnitude above theirs.
No mutation went unseen by the new rows."""
import pytest
import torch

from tests import adjoint_matrix as M
from tests import input_adjoint_matrix as IM
from tests import parity as P
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import ALBEDO_H2_CLASSES, FUSED_CLASSES, device, named, profile_classes

pytestmark = pytest.mark.gpu


def _build(R, shape):
    mc, p = M.model(shape)
    return R.build_from_named_params(mc, p, device())


def _run(R, nets, row, want, shared_lights=None, profile=False):
    """One render of the row's api at the table's depths with the inputs `want` requiring grad and the backward of the
    row's functional: (outputs, {input: gradient on the CPU}, {leaf: gradient on the CPU}, kernel classes or None)"""
    sdf, dev, col, ren = nets
    lib = R.native.load()
    params = named(sdf, dev, col)
    for v in params.values():
        v.grad = None
    b = {k: v.to(device()) for k, v in M.batch(row.shape, row.api).items()}
    x = {k: v.to(device()).detach().requires_grad_(k in want) for k, v in IM.input_values(row.shape, row.api, shared_lights).items()}
    classes = None
    if profile:
        lib.rnb_profile_enable(1)
    try:
        if row.api == "render":
            out = ren.render(x["rays_o"], x["rays_d"], b["near"], b["far"], background_rgb=x["background_rgb"],
                             cos_anneal_ratio=M.COS_ANNEAL, z_vals=x["z_vals"])
        else:
            fn = ren.render_rnb_warmup if row.api == "render_rnb_warmup" else ren.render_rnb
            out = fn(x["rays_o"], x["rays_d"], b["near"], b["far"], x["lights_dir"], cos_anneal_ratio=M.COS_ANNEAL,
                     no_albedo=row.api == "render_rnb_no_albedo", z_vals=x["z_vals"])
        assert torch.equal(ren.last_z_vals.cpu(), M.depths(row.shape)), "the render must run at the depths it was given"
        M.functional(row, out).backward()
        torch.cuda.synchronize()
        if profile:
            classes = profile_classes(R)
    finally:
        if profile:
            lib.rnb_profile_enable(0)
    for k in x:
        assert (x[k].grad is not None) == (k in want), f"{row.name}: {k}: gradient {'missing' if k in want else 'not asked for'}"
    grads = {k: x[k].grad.detach().cpu().clone() for k in want}
    leaves = {k: (None if v.grad is None else v.grad.detach().cpu().clone()) for k, v in params.items()}
    return out, grads, leaves, classes


def _assert_exact_zero(tag, k, g):
    assert bool(torch.isfinite(g).all()), f"{tag}: {k}: not finite"
    assert not bool((g != 0).any()), f"{tag}: {k}: no cotangent reaches it, yet max |gradient| is {float(g.abs().max()):.3e}, not 0.0"


def _check_inputs(row, mine, shared_lights=None, label=None):
    """every input gradient of the row by the gradient rule or to exact zero; one INADJROW line each; {input: rel / bound}"""
    tag = row.name if label is None else f"{row.name} [{label}]"
    g64 = IM.oracle_input_grads(row, torch.float64, shared_lights)
    g32 = IM.oracle_input_grads(row, torch.float32, shared_lights)
    assert set(mine) == set(g64)
    zero, dropped = IM.zero_inputs(row), IM.zero_rays(row)
    ratios = {}
    for k in IM.inputs(row):
        g = mine[k]
        if k in zero:
            _assert_exact_zero(tag, k, g)
            print(f"INADJROW {tag}: {k} exactly 0.0")
            continue
        assert g.shape == g64[k].shape, f"{tag}: {k} has shape {tuple(g.shape)}, not {tuple(g64[k].shape)}"
        assert bool(torch.isfinite(g).all()), f"{tag}: gradient of {k} is not finite"
        a, r64, r32 = g, g64[k], g32[k]
        note = ""
        if dropped is not None:
            _assert_exact_zero(f"{tag}: rows of the {int(dropped.sum())} dropped rays", k, g[dropped])
            a, r64, r32 = g[~dropped], r64[~dropped], r32[~dropped]
            note = f" on {int((~dropped).sum())} of {len(dropped)} rays, the other rows exactly 0.0"
        rel32 = P.rel_l2(r32, r64)
        print(f"INADJROW {tag}: {k} rel-L2 {P.rel_l2(a, r64):.2e} (bound {P.grad_bound(rel32):.2e}, |fp64| {float(r64.norm()):.2e}) = "
              f"{P.rel_l2(a, r64) / P.grad_bound(rel32):.2f} of its bound{note}")
        ratios[k] = P.check_grad(f"{tag}: {k}", a, r64, rel32)
    return ratios


def _check_outputs(row, out, shared_lights=None):
    o64 = IM.oracle_outputs(row.shape, row.api, torch.float64, shared_lights)
    o32 = IM.oracle_outputs(row.shape, row.api, torch.float32, shared_lights)
    if "weight_max" in row.outputs:
        # first: the device puts the cotangent on the sample the oracle puts it on
        kept, arg64, _ = M.weight_max_selection(row.shape)
        P.check_value(f"{row.name}: weights", out["weights"], o64["weights"], o32["weights"])
        arg = out["weights"].detach().cpu().argmax(dim=-1)
        assert torch.equal(arg[kept], arg64[kept]), \
            f"{row.name}: the device's arg-max differs from fp64 on kept rays {torch.nonzero(arg[kept] != arg64[kept]).flatten().tolist()}"
    for k in row.outputs:
        P.check_value(f"{row.name}: {k}", out[k], o64[k].reshape(out[k].shape), o32[k].reshape(out[k].shape))


# ------------------------------------------------------------------------------------------------------------ 1 the table
@pytest.mark.parametrize("row", IM.INPUT_ROWS, ids=[r.name for r in IM.INPUT_ROWS])
def test_row_against_fp64(R, row):
    out, mine, _, classes = _run(R, _build(R, row.shape), row, IM.inputs(row), profile=True)
    _check_outputs(row, out)
    _check_inputs(row, mine)
    if row.shape == "w32":
        assert "layer_gemm" in classes and not ((FUSED_CLASSES | ALBEDO_H2_CLASSES) & classes), sorted(classes)
    elif row.api == "render_rnb_no_albedo":
        assert FUSED_CLASSES <= classes and not (ALBEDO_H2_CLASSES & classes), sorted(classes)
    else:
        assert FUSED_CLASSES <= classes and ALBEDO_H2_CLASSES <= classes, sorted(classes)


# ------------------------------------------------------------------------------------------------------------- 2 variants
VARIANT_ROWS = ("default_64x64-render_rnb-all", "default_64x64-render_rnb-gradients", "default_64x64-render_rnb_no_albedo-color_fine")
VARIANTS = (
    dict(bwd_ti=1, bwd_nw=4),
    dict(bwd_ti=1, bwd_nw=8),
    dict(bwd_ti=2, bwd_nw=8),
    dict(f32_mfma=True),
    dict(f32_mfma=True, bwd_ti=2, bwd_nw=4),
    dict(x3=True),
    dict(x2h=False),
    dict(x2h=False, bwd_ti=1, bwd_nw=8),
    dict(deterministic=True),
    dict(generic=True),
)
ARITHMETIC = ("f32_mfma", "x2h", "generic")      # the switches that change the arithmetic: they must be seen to arrive


def _variant_id(v):
    return ",".join(f"{k}={x}" if not (x is True) else k for k, x in v.items())


@pytest.mark.parametrize("variant", VARIANTS, ids=_variant_id)
@pytest.mark.parametrize("name", VARIANT_ROWS)
def test_variant_against_fp64(R, name, variant):
    row = IM.BY_NAME[name]
    nets = _build(R, row.shape)
    ren = nets[3]
    default = None
    if any(k in variant for k in ARITHMETIC):
        _, default, _, default_classes = _run(R, nets, row, IM.inputs(row), profile=True)
        assert "R_sweep" in default_classes, sorted(default_classes)
    ren.set_variant(**variant)
    try:
        out, mine, _, classes = _run(R, nets, row, IM.inputs(row), profile=True)
    finally:
        ren.set_variant()
    _check_outputs(row, out)
    _check_inputs(row, mine, label=_variant_id(variant))
    if "generic" in variant:
        assert "layer_gemm" in classes and "R_sweep" not in classes, sorted(classes)
    else:
        # (layer_gemm does not tell these apart: off the x2h arithmetic the albedo network runs as layer GEMMs behind the sweeps)
        assert "R_sweep" in classes, sorted(classes)
        if default is not None:
            live = [k for k in mine if k not in IM.zero_inputs(row)]
            assert not all(torch.equal(mine[k], default[k]) for k in live), \
                f"{name} [{_variant_id(variant)}]: no input gradient differs in bits from the default variant's: the switch did not arrive"


# -------------------------------------------------------------------------------------------------------------- 3 subsets
@pytest.mark.parametrize("api", ["render_rnb", "render"])
def test_subsets_of_wanted_inputs(R, api):
    """The kernels branch on which fields of rnb_render_input_grads are non-NULL (ig_cos_d, ig_dists, need_pbar, cos_d,
    dists_bar).  Each input alone and two pairs: every gradient bit-equal to the one of the call that wants them all, the
    parameter gradients bit-equal to the call that wants none.  (default_64x64: every reduction of the fused path has a
    fixed order.)"""
    row = IM.BY_NAME[f"default_64x64-{api}-all"]
    nets = _build(R, row.shape)
    every = IM.inputs(row)
    colour_input = every[3]
    assert colour_input in ("lights_dir", "background_rgb")
    _, full, leaves_full, _ = _run(R, nets, row, every)
    _, none, leaves_none, _ = _run(R, nets, row, ())
    assert none == {}
    subsets = [(k,) for k in every] + [("rays_o", "z_vals"), ("rays_d", colour_input)]
    for k in every:
        assert float(full[k].abs().max()) > 0.0
    for want in [every] + subsets:
        _, mine, leaves, _ = _run(R, nets, row, want)
        assert set(mine) == set(want)
        for k in want:
            assert torch.equal(mine[k], full[k]), \
                f"{api}: {k} wanted with {want} differs from all-wanted by up to {float((mine[k] - full[k]).abs().max()):.3e}"
        assert set(leaves) == set(leaves_none)
        for k, g in leaves_none.items():
            assert g is not None and leaves[k] is not None, f"{api} {want}: {k}: no gradient"
            assert torch.equal(leaves[k], g), \
                f"{api}: parameter gradient {k} with inputs {want} differs from no-inputs by up to {float((leaves[k] - g).abs().max()):.3e}"


# ------------------------------------------------------------------------------------------- 4 lights on the no-albedo branch
@pytest.mark.parametrize("shared", [False, True], ids=["per_ray", "shared"])
def test_no_albedo_lights_of_both_shapes(R, shared):
    """render_rnb(no_albedo=True) under color_fine with [L,B,1,3] and with [L,1,1,3] lights (sum_over_rays_kernel behind the
    `cinb == nullptr` branch): lights_dir.grad of both shapes, and the ray inputs, by the gradient rule"""
    row = IM.BY_NAME["default_64x64-render_rnb_no_albedo-color_fine"]
    out, mine, _, _ = _run(R, _build(R, row.shape), row, IM.inputs(row), shared_lights=shared)
    assert tuple(mine["lights_dir"].shape) == ((3, 1, 1, 3) if shared else (3, 64, 1, 3))
    _check_outputs(row, out, shared)
    _check_inputs(row, mine, shared, label="shared lights" if shared else "per-ray lights")
