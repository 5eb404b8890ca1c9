"""Parameter gradients under each cotangent of a render alone (rnb_render_grads: color_fine, weights, cdf_fine, gradients,
weight_sum, weight_max, s_val, gradient_error), against the fp64 oracle, over the table of tests/adjoint_matrix.py.

Every other device-vs-fp64 comparison of parameter gradients drives the backward with the training loss, which feeds
color_fine, gradient_error and weight_sum only.  Here each row renders at the table's explicit depths, takes the backward
of sum(cotangent . out[adjoint]) and holds
  every leaf the adjoint reaches (dev.variance among them) to the gradient rule of tests/parity.py,
  every leaf it cannot reach to a finite, exact 0.0 (a zero adjoint multiplies and sums to zero exactly in
  composite_bwd_body, in the sweeps and in rnb_weightnorm_bwd),
  the kernel classes to the shape's path.
The inputs are free of kinks before any device code runs (tests/test_adjoint_matrix_host.py): the weight_max cotangent is
zero on the rays whose top two weights lie within the output rule's reach of each other, and on the others the device's
arg-max must be the fp64 one.  Every row prints one line starting with ADJROW.

What the rows see, measured with one-line mutations of composite.hip: the sign of the s_val term, the weight_max cotangent
put one sample before the arg-max, component 1 for 2 of the gradients cotangent and the variance clip's `inside ? ... : 0`
removed each turn every row of their adjoint red on both shapes (and "all").  The weights cotangent read one sample off in
the ragged second chunk turns the default_64x64 rows red and not the w32 ones, whose samples 64 .. 79 lie behind the surface
(T ~ 0: their wbar reaches nothing).  Whether cdf_fine's cotangent is added after or inside the alpha clip's mask cannot be
seen by any finite input with sorted depths: iter_cos <= 0 makes next_cdf <= prev_cdf, so the raw alpha lies in (0, 1] and the mask is all ones.

After the table: no cotangent at all, explicit zero tensors against NULL, non-contiguous cotangents, and the variance
clip (inv_s = exp(10 variance).clip(1e-6, 1e6)) on both of its sides."""
import pytest
import torch

from tests import adjoint_matrix as M
from tests import parity as P
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import ALBEDO_H2_CLASSES, FUSED_CLASSES, device, named, profile_classes

pytestmark = pytest.mark.gpu


def _build(R, shape, params=None, reproducible=False):
    """`reproducible`: for the cases that compare two backward passes bit for bit.  The per-layer path's weight and bias
    gradients are fp32 atomics in the default variant (two runs of one step differ in the last bit), so w32 takes
    set_variant(deterministic=True) there; the fused path's reductions have a fixed order as they are."""
    mc, p = M.model(shape)
    sdf, dev, col, ren = R.build_from_named_params(mc, p if params is None else params, device())
    if reproducible and shape == "w32":
        ren.set_variant(deterministic=True)
    return sdf, dev, col, ren


def _render(ren, shape, api):
    b = {k: v.to(device()) for k, v in M.batch(shape, api).items()}
    z = M.depths(shape).to(device())
    if api == "render":
        out = ren.render(b["rays_o"], b["rays_d"], b["near"], b["far"], background_rgb=torch.tensor(M.BACKGROUND, device=device()),
                         cos_anneal_ratio=M.COS_ANNEAL, z_vals=z)
    else:
        fn = ren.render_rnb_warmup if api == "render_rnb_warmup" else ren.render_rnb
        out = fn(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=M.COS_ANNEAL,
                 no_albedo=api == "render_rnb_no_albedo", z_vals=z)
    assert torch.equal(ren.last_z_vals.cpu(), M.depths(shape)), "the render must run at the depths it was given"
    return out, b


def _clear(params):
    for v in params.values():
        v.grad = None


def _grads(params):
    return {k: (None if v.grad is None else v.grad.detach().cpu().clone()) for k, v in params.items()}


def _assert_exact_zero(tag, k, g):
    assert g is not None, f"{tag}: {k}: no gradient"
    assert bool(torch.isfinite(g).all()), f"{tag}: {k}: not finite"
    assert not bool((g != 0).any()), f"{tag}: {k}: a leaf no cotangent reaches has max |gradient| {float(g.abs().max()):.3e}, not 0.0"


# ------------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("row", M.ROWS, ids=[r.name for r in M.ROWS])
def test_row_against_fp64(R, row):
    lib = R.native.load()
    sdf, dev, col, ren = _build(R, row.shape)
    params = named(sdf, dev, col)
    _clear(params)
    lib.rnb_profile_enable(1)
    try:
        out, _ = _render(ren, row.shape, row.api)
        M.functional(row, out).backward()
        torch.cuda.synchronize()
        classes = profile_classes(R)
    finally:
        lib.rnb_profile_enable(0)
    mine = _grads(params)
    g64 = M.oracle_grads(row, torch.float64)
    g32 = M.oracle_grads(row, torch.float32)
    o64 = M.oracle_outputs(row.shape, row.api, torch.float64)
    o32 = M.oracle_outputs(row.shape, row.api, torch.float32)
    tag = row.name
    kept_note = ""
    if "weight_max" in row.outputs:
        # first: the device puts the cotangent on the sample the oracle puts it on
        kept, arg64, margin = M.weight_max_selection(row.shape)
        P.check_value(f"{tag}: weights", out["weights"], o64["weights"], o32["weights"])
        arg = out["weights"].detach().cpu().argmax(dim=-1)
        assert torch.equal(arg[kept], arg64[kept]), \
            f"{tag}: the device's arg-max differs from fp64 on kept rays {torch.nonzero(arg[kept] != arg64[kept]).flatten().tolist()}"
        kept_note = f"; weight_max cotangent on {int(kept.sum())} of {len(kept)} rays (top-two gap > {margin:.2e})"
    for k in row.outputs:
        P.check_value(f"{tag}: {k}", out[k], o64[k].reshape(out[k].shape), o32[k].reshape(out[k].shape))
    zero = M.zero_leaves(row)
    assert set(g64) == set(params)
    worst = ("", 0.0, 0.0)
    for k, g in g64.items():
        if k in zero:
            if row.api == "render_rnb_no_albedo" and mine[k] is None:
                continue      # no_albedo: the albedo network is not a leaf of the call, autograd hands it no gradient at all
            _assert_exact_zero(tag, k, mine[k])
            continue
        assert mine[k] is not None, f"{tag}: {k}: no gradient"
        assert bool(torch.isfinite(mine[k]).all()), f"{tag}: gradient of {k} is not finite"
        rel32 = P.rel_l2(g32[k], g)
        ratio = P.check_grad(f"{tag}: {k}", mine[k].reshape(g.shape), g, rel32)
        if ratio > worst[1]:
            worst = (k, ratio, P.rel_l2(mine[k].reshape(g.shape), g))
    assert M.VARIANCE in zero or mine[M.VARIANCE] is not None
    print(f"ADJROW {row.name} S={M.S}: {len(g64) - len(zero)} leaves by the gradient rule, {len(zero)} exactly zero; worst "
          f"{worst[0]} rel-L2 {worst[2]:.2e} = {worst[1]:.2f} of its bound{kept_note}; classes {sorted(classes)}")
    if row.shape == "w32":
        assert "layer_gemm" in classes and not ((FUSED_CLASSES | ALBEDO_H2_CLASSES) & classes), sorted(classes)
    else:
        assert FUSED_CLASSES <= classes and ALBEDO_H2_CLASSES <= classes, sorted(classes)


# ------------------------------------------------------------------------------------------------- NULL, zero, strided
class _NoGradient(torch.autograd.Function):
    """an op whose backward hands its input no gradient: what reaches the render's backward is an undefined cotangent"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return None


@pytest.mark.parametrize("shape", list(M.RAYS))
def test_no_cotangent_at_all_gives_exact_zeros(R, shape):
    """every cotangent NULL (rnb_render_grads: "NULL means zero"): the backward runs and every leaf reads exactly 0.0"""
    sdf, dev, col, ren = _build(R, shape)
    params = named(sdf, dev, col)
    _clear(params)
    out, _ = _render(ren, shape, "render_rnb")
    _NoGradient.apply(out["color_fine"]).sum().backward()
    torch.cuda.synchronize()
    for k, g in _grads(params).items():
        _assert_exact_zero(f"{shape}: no cotangent", k, g)


def _backward_with(ren, params, shape, api, cots):
    """render, backward with the cotangents given ({output: tensor on the device}); the parameter gradients on the CPU"""
    _clear(params)
    out, _ = _render(ren, shape, api)
    keys = list(cots)
    torch.autograd.backward([out[k] for k in keys], [cots[k] for k in keys])
    torch.cuda.synchronize()
    return _grads(params)


def _assert_bit_equal(tag, a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k] is not None and b[k] is not None, f"{tag}: {k}: no gradient"
        assert bool(torch.isfinite(a[k]).all()), f"{tag}: {k}: not finite"
        assert torch.equal(a[k], b[k]), f"{tag}: {k} differs by up to {float((a[k] - b[k]).abs().max()):.3e}"


@pytest.mark.parametrize("shape", list(M.RAYS))
@pytest.mark.parametrize("adjoint", ["color_fine", "cdf_fine"])
def test_zero_tensors_equal_null_cotangents(R, shape, adjoint):
    """one live cotangent with the seven others NULL, against the same with the seven others as tensors of zeros"""
    api = "render_rnb"
    sdf, dev, col, ren = _build(R, shape, reproducible=True)
    params = named(sdf, dev, col)
    cot = {k: v.to(device(), torch.float32) for k, v in M.cotangents(shape, api).items()}
    with_null = _backward_with(ren, params, shape, api, {adjoint: cot[adjoint]})
    with_zeros = _backward_with(ren, params, shape, api,
                                {k: (cot[k] if k == adjoint else torch.zeros_like(cot[k])) for k in M.ADJOINTS})
    assert float(with_null["sdf.lin0.weight_v"].abs().max()) > 0.0
    _assert_bit_equal(f"{shape} {adjoint}: zeros against NULL", with_zeros, with_null)


@pytest.mark.parametrize("shape", list(M.RAYS))
def test_non_contiguous_cotangents(R, shape):
    """What _FinePass.backward's gp() receives is not always contiguous.  (a) the loss weight_sum.sum() +
    weights[:, ::2].sum(): autograd hands weight_sum a stride-0 expanded cotangent; (b) cotangents given directly as a
    column-strided view (weights), a permuted one (gradients) and an expanded one (color_fine).  Both against the same
    values materialised contiguously, bit for bit."""
    api = "render_rnb"
    B, _ = M.RAYS[shape]
    sdf, dev, col, ren = _build(R, shape, reproducible=True)
    params = named(sdf, dev, col)
    d = device()
    # (a)
    _clear(params)
    out, _ = _render(ren, shape, api)
    (out["weight_sum"].sum() + out["weights"][:, ::2].sum()).backward()
    torch.cuda.synchronize()
    from_loss = _grads(params)
    w_cot = torch.zeros(B, M.S, device=d)
    w_cot[:, ::2] = 1.0
    plain = _backward_with(ren, params, shape, api, {"weight_sum": torch.ones(B, 1, device=d), "weights": w_cot})
    _assert_bit_equal(f"{shape}: expanded cotangent from a loss", from_loss, plain)
    # (b)
    g = torch.Generator().manual_seed(17)
    L = M.batch(shape, api)["lights_dir"].shape[0]
    strided = {
        "weights": (torch.randn(B, 2 * M.S, generator=g) / (B * M.S) ** 0.5).to(d)[:, ::2],
        "gradients": (torch.randn(3, B, M.S, generator=g) / (3 * B * M.S) ** 0.5).to(d).permute(1, 2, 0),
        "color_fine": (torch.randn(1, B, 1, generator=g) / B ** 0.5).to(d).expand(L, B, 3),
    }
    assert not any(t.is_contiguous() for t in strided.values())
    got = _backward_with(ren, params, shape, api, strided)
    want = _backward_with(ren, params, shape, api, {k: t.contiguous() for k, t in strided.items()})
    assert float(want["color.lin0.weight_v"].abs().max()) > 0.0
    _assert_bit_equal(f"{shape}: strided cotangents", got, want)


# ------------------------------------------------------------------------------------------------------ variance clip
@pytest.mark.parametrize("variance,inside", M.CLIP_VARIANCES)
def test_variance_clip(R, variance, inside):
    """w32 at dev.variance = +-1.3815 (raw inv_s 9.995e5 / 1.0005e-6: inside the clip) and +-1.4 (outside), under the
    training loss plus sum(s_val): outputs by the output rule, parameter gradients by the gradient rule; outside the clip
    s_val reads the clip value and d loss / d variance is exactly 0 (variance_grad_kernel's `inside ? ... : 0`)."""
    shape, api = M.CLIP_SHAPE, M.CLIP_API
    sdf, dev, col, ren = _build(R, shape, M.clip_params(variance))
    params = named(sdf, dev, col)
    _clear(params)
    out, b = _render(ren, shape, api)
    M.clip_loss(out, b).backward()
    torch.cuda.synchronize()
    mine = _grads(params)
    o64, g64 = M.clip_oracle(variance, torch.float64)
    o32, g32 = M.clip_oracle(variance, torch.float32)
    tag = f"clip variance {variance:+.4f}"
    worst_out = ("", 0.0)
    for k in M.ADJOINTS:
        ratio = P.check_value(f"{tag}: {k}", out[k], o64[k].reshape(out[k].shape), o32[k].reshape(out[k].shape))
        if ratio > worst_out[1]:
            worst_out = (k, ratio)
    if not inside:
        # one rounding in the clip's constant, one in the division: two fp32 ulps
        want = 1e-6 if variance > 0 else 1e6
        torch.testing.assert_close(out["s_val"].detach().cpu().double(), torch.full((M.RAYS[shape][0], 1), want, dtype=torch.float64),
                                   rtol=2.4e-7, atol=0.0)
    worst = ("", 0.0)
    for k, g in g64.items():
        if k == M.VARIANCE and not inside:
            _assert_exact_zero(tag, k, mine[k])
            continue
        assert mine[k] is not None and bool(torch.isfinite(mine[k]).all()), f"{tag}: gradient of {k} is missing or not finite"
        ratio = P.check_grad(f"{tag}: {k}", mine[k].reshape(g.shape), g, P.rel_l2(g32[k], g))
        if ratio > worst[1]:
            worst = (k, ratio)
    if inside:
        assert float(mine[M.VARIANCE].abs().max()) > 0.0
    print(f"ADJROW {tag} ({'inside' if inside else 'outside'}): s_val {float(out['s_val'].detach()[0, 0]):.6e}, d loss / d variance "
          f"{float(mine[M.VARIANCE]):.6e} (fp64 {float(g64[M.VARIANCE]):.6e}); worst output {worst_out[0]} {worst_out[1]:.2f}, "
          f"worst gradient {worst[0]} {worst[1]:.2f} of its bound")
