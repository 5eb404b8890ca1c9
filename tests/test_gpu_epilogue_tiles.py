"""The sweeps whose epilogues were rearranged around the vector-memory counter (csrc/color_h2.hip, csrc/fused.hip: what a
phase loads is requested ahead of its stores), on the full-width networks at tiny point counts.

Tiles are independent: a 64-point tile's results depend on its own rows only.  A stale register or LDS value left behind by a
restructured phase therefore shows up as a difference in the FIRST tile between two point counts (one tile; one tile and a
one-row ragged tile; more tiles), and a phase that reads what an earlier one has not finished writing as a difference between
two runs.  The first 64 rows are compared bit for bit (torch.equal); the one-row ragged tiles and the render step are held to
the fp64 oracle by the rule of tests/parity.py, unchanged."""
from dataclasses import replace

import pytest
import torch

from oracle import rnb_oracle as O
from tests.field_autograd_util import build, check_grad_or_zero, native_leaf_grads, oracle, weights, zero_grads
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import ALBEDO_H2_CLASSES, device, profile_classes, step_against_fp64
from tests.shape_matrix import BY_NAME as SHAPE_BY_NAME, live_params, points

pytestmark = pytest.mark.gpu

SHAPE = "default_64x64"
ALBEDO_COUNTS = (64, 65, 129)      # one tile; one tile + a one-row tile; two tiles + a one-row tile
FORWARD_COUNTS = (64, 65, 200)
M_MAX = 129
INPUT_NAMES = ("points", "normals", "feats")


@pytest.fixture(scope="module")
def nets(R):
    return build(R, SHAPE)


@pytest.fixture(scope="module")
def albedo_inputs(nets):
    """(points, normals, feats, adjoint weights) of M_MAX rows: a run at M rows takes the first M of each"""
    shape = nets[0]
    return (points(M_MAX, seed=71), torch.nn.functional.normalize(weights(M_MAX, 3, 3), dim=-1),
            0.5 * weights(M_MAX, shape.mc.color.d_feature, 4), weights(M_MAX, shape.mc.color.d_out, 5))


def albedo_backward(R, nets, inputs, M):
    """(pts_bar, nrm_bar, feat_bar) of loss = sum(W * albedo) through the direct albedo-net call at the first M rows"""
    shape, p, sdf, col, ren = nets
    zero_grads(sdf, col)
    xs = [t[:M].to(device()).requires_grad_(True) for t in inputs[:3]]
    lib = R.native.load()
    lib.rnb_profile_enable(1)
    try:
        out = col(xs[0], xs[1], xs[1].detach(), xs[2])
        (inputs[3][:M].to(device()) * out).sum().backward()
        torch.cuda.synchronize()
        classes = profile_classes(R)
    finally:
        lib.rnb_profile_enable(0)
    assert ALBEDO_H2_CLASSES <= classes, f"M={M}: the albedo sweeps did not run: {sorted(classes)}"
    return [t.grad.clone() for t in xs]


@pytest.fixture(scope="module")
def albedo_grads(R, nets, albedo_inputs):
    """{M: input adjoints} of the first run at every point count (shared by the tests below, never modified)"""
    return {M: albedo_backward(R, nets, albedo_inputs, M) for M in ALBEDO_COUNTS}


def test_albedo_backward_first_tile_is_the_same_at_every_point_count(albedo_grads):
    base = albedo_grads[ALBEDO_COUNTS[0]]
    for M in ALBEDO_COUNTS[1:]:
        for name, a, b in zip(INPUT_NAMES, base, albedo_grads[M]):
            assert bool(a[:64].abs().max() > 0), f"{name}.grad vanishes: nothing to compare"
            assert torch.equal(a[:64], b[:64]), \
                f"{name}.grad[:64] differs between M={ALBEDO_COUNTS[0]} and M={M}: max |d| {float((a[:64] - b[:64]).abs().max()):.3e}"


@pytest.mark.parametrize("M", ALBEDO_COUNTS)
def test_albedo_backward_twice_bit_for_bit(R, nets, albedo_inputs, albedo_grads, M):
    again = albedo_backward(R, nets, albedo_inputs, M)
    for name, a, b in zip(INPUT_NAMES, albedo_grads[M], again):
        assert torch.equal(a, b), f"M={M}: {name}.grad differs between two runs: max |d| {float((a - b).abs().max()):.3e}"


@pytest.fixture(scope="module")
def albedo_oracle(nets, albedo_inputs):
    """input adjoints of the torch oracle at M_MAX rows in fp64 and fp32 (a row's adjoint does not depend on the other rows:
    the loss is a sum over rows)"""
    shape, p = nets[0], nets[1]
    W = albedo_inputs[3]

    def fn(q, x, n, f):
        out = O.color_forward(q, shape.mc.color, x, n, n, f)
        return out, (W.to(out) * out).sum()
    return {dt: oracle(p, "color.", albedo_inputs[:3], fn, dt)[2] for dt in (torch.float64, torch.float32)}


@pytest.mark.parametrize("M", (65, 129))
def test_albedo_backward_one_row_tile_against_fp64(albedo_grads, albedo_oracle, M):
    """row M - 1 is alone in its tile (rows_ok = 1): its adjoints come from a tile whose other 63 rows are padding"""
    i64, i32 = albedo_oracle[torch.float64], albedo_oracle[torch.float32]
    for name, got, r64, r32 in zip(INPUT_NAMES, albedo_grads[M], i64, i32):
        ratio = check_grad_or_zero(got[M - 1:M].cpu(), r64[M - 1:M].cpu(), r32[M - 1:M].cpu(), f"M={M} {name}.grad, row {M - 1}")
        print(f"EPITILE albedo backward M={M} {name}.grad row {M - 1}: {ratio:.2f} of its bound")


def test_render_backward_albedo_gradients(R):
    """2 rays x (32 + 32) samples: the backward of a render runs the albedo sweep with the RA sweep's input (geb) behind it.
    Rays of synthetic_batch(seed 11, step 3): the fp32 oracle renders weight_sum 0.70 and 0.80 on them.  Every parameter
    gradient against the fp64 oracle at the bounds of tests/parity.py; the albedo net's twice, bit for bit."""
    shape = SHAPE_BY_NAME[SHAPE]
    mc = replace(shape.mc, render=O.RenderConf(n_samples=32, n_importance=32))
    p = live_params(mc, shape.seed)
    sdf, dev, col, ren = R.build_from_named_params(mc, p, device())
    batch = O.synthetic_batch(2, seed=11, step=3, warmup=False)
    stats = {}
    lib = R.native.load()
    lib.rnb_profile_enable(1)
    try:
        step_against_fp64(R, mc, p, sdf, dev, col, ren, batch, "epilogue tiles, 2 rays x 64", survey=False, stats=stats,
                          loss_rule="calibrated")
        classes = profile_classes(R)
    finally:
        lib.rnb_profile_enable(0)
    assert ALBEDO_H2_CLASSES <= classes and "RA_sweep" in classes, sorted(classes)
    assert stats["n_checked"] == len(O.param_order(mc))
    first = {k: v.clone() for k, v in native_leaf_grads(col, "color").items()}
    z = ren.last_z_vals.clone()
    zero_grads(sdf, col)
    dev.variance.grad = None
    b = {k: v.to(device()) for k, v in batch.items()}
    out = ren.render_rnb(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=1.0, t_rand=b["t_rand"])
    O.rnb_loss(out, b["true_rgb"], b["mask"])[0].backward()
    torch.cuda.synchronize()
    assert torch.equal(ren.last_z_vals, z), "the two runs sampled different depths"
    for k, v in native_leaf_grads(col, "color").items():
        assert torch.equal(v, first[k]), f"{k}: gradient differs between two runs: max |d| {float((v - first[k]).abs().max()):.3e}"


def _set_variant(monkeypatch, R, **variant):
    """the direct calls build their own descriptors (runtime.model_desc / _color_desc): the variant bits go in there"""
    bits = R.native.variant_bits(**variant)
    for name in ("model_desc", "_color_desc"):
        plain = getattr(R.runtime, name)

        def with_bits(*a, _plain=plain, **k):
            d = _plain(*a, **k)
            d.variant = bits
            return d
        monkeypatch.setattr(R.runtime, name, with_bits)


# (tile height, waves): the 64-point tile kernel; the 32-point one as small batches get it (8 waves) and with 4 waves
FORWARD_KERNELS = [(2, 4), (1, 8), (1, 4)]


@pytest.mark.parametrize("save", (False, True), ids=("forward_only", "save"))
@pytest.mark.parametrize("ti,nw", FORWARD_KERNELS, ids=[f"ti{t}_nw{n}" for t, n in FORWARD_KERNELS])
def test_sdf_forward_first_tile_is_the_same_at_every_point_count(R, nets, monkeypatch, ti, nw, save):
    """SDFNetwork.forward (sdf and feature columns) of the first 64 points at M = 64, 65, 200, on each forward kernel, without
    and with the saved state of a backward"""
    shape, p, sdf, col, ren = nets
    _set_variant(monkeypatch, R, fwd_ti=ti, fwd_nw=nw)
    x = points(FORWARD_COUNTS[-1], seed=83).to(device())
    lib = R.native.load()
    outs = {}
    lib.rnb_profile_enable(1)
    try:
        for M in FORWARD_COUNTS:
            if save:
                outs[M] = sdf(x[:M].clone().requires_grad_(True)).detach()
            else:
                with torch.no_grad():
                    outs[M] = sdf(x[:M])
        torch.cuda.synchronize()
        classes = profile_classes(R)
    finally:
        lib.rnb_profile_enable(0)
    want = "F_sweep(save)" if save else "F_sweep(forward_only)"
    assert want in classes, f"{want} did not run: {sorted(classes)}"
    base = outs[FORWARD_COUNTS[0]]
    assert base.shape == (64, shape.mc.sdf.d_out) and bool(torch.isfinite(base).all()) and bool(base[:, 1:].abs().max() > 0)
    for M in FORWARD_COUNTS[1:]:
        assert torch.equal(base, outs[M][:64]), \
            f"ti={ti} nw={nw}: rows 0 .. 63 differ between M=64 and M={M}: max |d| {float((base - outs[M][:64]).abs().max()):.3e}"
