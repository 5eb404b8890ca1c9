"""Every network shape of tests/shape_matrix.py against the oracle in fp64, on the device.

The fused x2h kernels are compiled for a 256-wide network but read the skip position, pe, Ep, the layer count, the feature
width and the SDF scale at run time; the per-layer GEMMs take any width.  Each shape runs here in a live state
(shape_matrix.live_params: no zero block, so the PE columns of lin0 and of the skip layer carry a share of every Jacobian)
with the calibrated rule of tests/parity.py (K_OUT, FLOOR_OUT for outputs; K_GRAD, GRAD_CAP for gradients):
  - point-wise SDF + feature, normal and albedo at 1, 63 and 4097 points, at both tile heights of the fused sweeps and,
    where sweep_mv_supported holds, through the M/V kernels (RNB_VARIANT_REG_TILE);
  - one end-to-end train step (sampling, fine pass, loss, backward; every parameter gradient), with the kernel classes it
    launched read back from the library's profiler, so that a shape cannot pass on a path other than the one tabled;
  - rnb_sdf_grid on four shapes; RNB_VARIANT_BF16 against oracle/bf16_emu.py on four.
Every case prints one line: the path classes and the worst error as a fraction of its bound."""
import ctypes as C

import pytest
import torch

from oracle import rnb_oracle as O
from tests.bf16_emu_step import linspace_at, step as bf16_step
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import ALBEDO_H2_CLASSES, FUSED_CLASSES, device, profile_classes, step_against_fp64
from tests.parity import check_value
from tests.shape_matrix import BY_NAME, SHAPES, live_params, oracle_points, points, step_batch

pytestmark = pytest.mark.gpu

RENDER_SHAPES = [s for s in SHAPES if s.render]


def _build(R, shape):
    p = live_params(shape.mc, shape.seed)
    sdf, dev, col, ren = R.build_from_named_params(shape.mc, p, device())
    return p, sdf, dev, col, ren


def _point_variants(shape):
    """(tag, variant keywords) of the point-wise queries: both tile heights of the fused sweeps (TI 1: 32 rows, 2: 64 rows)
    and, where sweep_mv_supported holds, the M/V forward kernels; the generic path has one form"""
    if not shape.fused:
        return [("generic", {})]
    out = [("ti1", dict(fwd_ti=1, bwd_ti=1)), ("ti2", dict(fwd_ti=2, bwd_ti=2))]
    if shape.mv:
        out.append(("mv", dict(reg_tile=True)))
    return out


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("shape", SHAPES, ids=[s.name for s in SHAPES])
def test_pointwise_against_fp64(R, shape):
    mc = shape.mc
    p, sdf, dev, col, ren = _build(R, shape)
    F = mc.sdf.d_out - 1
    worst = {}
    for n in (1, 63, 4097):
        pts = points(n, seed=n)
        gen = torch.Generator().manual_seed(n + 1)
        nrm = torch.randn(n, 3, generator=gen)
        feats = torch.randn(n, F, generator=gen) * 0.3
        r64 = oracle_points(p, mc, pts, nrm, feats, torch.float64)
        r32 = oracle_points(p, mc, pts, nrm, feats, torch.float32)
        for vtag, kw in _point_variants(shape):
            desc = R.model_desc(sdf, col)
            desc.variant = R.native.variant_bits(**kw)
            with torch.no_grad():
                packed = R.runtime.pack_weights(desc, sdf, col, device())
                out = R.runtime.sdf_forward(desc, packed, pts.to(device()), True)
                only = R.runtime.sdf_forward(desc, packed, pts.to(device()), False)
                grad = R.runtime.sdf_gradient(desc, packed, pts.to(device()))
                alb = R.runtime.color_forward(desc, packed, pts.to(device()), nrm.to(device()), feats.to(device()))
            torch.cuda.synchronize()
            tag = f"{shape.name} {vtag} n={n}"
            assert torch.equal(only, out[:, :1]), f"{tag}: sdf-only and sdf + feature sweeps must agree bit for bit"
            for what, got, a64, a32 in (("sdf", out[:, :1], r64[0][:, :1], r32[0][:, :1]),
                                        ("feature", out[:, 1:], r64[0][:, 1:], r32[0][:, 1:]),
                                        ("normal", grad, r64[1], r32[1]), ("albedo", alb, r64[2], r32[2])):
                r = check_value(f"{tag}: {what}", got, a64, a32)
                if r >= worst.get(vtag, ("", -1.0))[1]:
                    worst[vtag] = (f"{what} n={n}", r)
    print(f"SHAPE {shape.name} point-wise [{shape.path}]: " + "; ".join(
        f"{v}: worst {w[0]} {w[1]:.2f} of its bound" for v, w in worst.items()))


# ---------------------------------------------------------------------------------------------------------------- 2
def _step_variants(shape):
    """M/V and LDS-tile kernels differ only in the forward-only sweeps (the sampling passes), and the profile does not
    tell them apart: where sweep_mv_supported holds (Ep = 64, 2..8 hidden layers of >= 192 outputs, a 256-row feature head
    of a width divisible by 4) the step runs once with each"""
    if shape.mv:
        return [("lds_tile", dict(lds_tile=True)), ("reg_tile", dict(reg_tile=True))]
    return [("default", {})]


@pytest.mark.parametrize("shape", RENDER_SHAPES, ids=[s.name for s in RENDER_SHAPES])
def test_train_step_against_fp64(R, shape):
    lib = R.native.load()
    for vtag, kw in _step_variants(shape):
        p, sdf, dev, col, ren = _build(R, shape)
        ren.set_variant(**kw)
        stats = {}
        tag = f"{shape.name} {vtag}"
        lib.rnb_profile_enable(1)
        try:
            step_against_fp64(R, shape.mc, p, sdf, dev, col, ren, step_batch(), tag, survey=False, stats=stats)
            classes = profile_classes(R)
        finally:
            lib.rnb_profile_enable(0)
        print(f"SHAPE {tag} step [{shape.path}]: classes {sorted(classes)}; worst output {stats['worst_out'][0]} "
              f"{stats['worst_out'][1]:.2f}, worst gradient {stats['worst_grad'][0]} {stats['worst_grad'][1]:.2f} of its bound")
        if shape.fused:
            assert FUSED_CLASSES <= classes, f"{tag}: fused sweeps missing: {sorted(FUSED_CLASSES - classes)}"
            if shape.color_h2:
                assert ALBEDO_H2_CLASSES <= classes, f"{tag}: the fused albedo sweeps (color_h2) did not run"
            else:
                assert not (ALBEDO_H2_CLASSES & classes), f"{tag}: color_h2 ran on a shape it does not support"
                assert "layer_gemm" in classes, f"{tag}: the albedo network's layer GEMMs did not run"
        else:
            assert "layer_gemm" in classes, f"{tag}: the per-layer GEMMs did not run"
            assert not ((FUSED_CLASSES | ALBEDO_H2_CLASSES) & classes), f"{tag}: a fused kernel ran on a generic shape"
        assert stats["n_checked"] == len(O.param_order(shape.mc))


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", ["no_skip", "multires0", "scale3", "w100"])
def test_sdf_grid_against_fp64(R, name):
    """rnb_sdf_grid (odd resolution, an x-slab) against the oracle on the coordinates the kernel generates"""
    shape = BY_NAME[name]
    p, sdf, dev, col, ren = _build(R, shape)
    lib = R.native.load()
    res, x0, x1 = 37, 5, 30
    lo, hi = [-1.0, -0.9, -0.8], [1.0, 0.9, 1.1]
    gd = R.native.GridDesc()
    for d in range(3):
        gd.bound_min[d], gd.bound_max[d] = lo[d], hi[d]
    gd.resolution, gd.x_begin, gd.x_end, gd.out_scale = res, x0, x1, -1.0
    packed = ren._pack(False)
    vol = torch.full((x1 - x0, res, res), float("nan"), dtype=torch.float32, device=device())
    nbytes = C.c_int64()
    R.native.check(lib.rnb_sdf_grid_workspace_bytes(C.byref(ren.desc), C.byref(gd), C.byref(nbytes)))
    ws = torch.empty(max(nbytes.value, 256), dtype=torch.uint8, device=device())
    with R.native.on_device(vol) as stream:
        R.native.check(lib.rnb_sdf_grid(C.byref(ren.desc), R.native.ptr(packed), C.byref(gd), R.native.ptr(vol),
                                        R.native.ptr(ws), ws.numel(), stream))
    torch.cuda.synchronize()
    xs = [linspace_at(lo[0], hi[0], res, torch.arange(x0, x1)), linspace_at(lo[1], hi[1], res, torch.arange(res)),
          linspace_at(lo[2], hi[2], res, torch.arange(res))]
    xx, yy, zz = torch.meshgrid(*xs, indexing="ij")
    pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], dim=-1)
    ref = {}
    for dt in (torch.float64, torch.float32):
        q = {k: v.to(dt) for k, v in p.items()}
        with torch.no_grad():
            ref[dt] = -O.sdf_forward(q, shape.mc.sdf, pts.to(dt))[:, :1].reshape(vol.shape)
    r = check_value(f"grid {name}: sdf", vol, ref[torch.float64], ref[torch.float32])
    print(f"SHAPE {name} sdf_grid [{shape.path}]: worst {r:.2f} of its bound")


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", ["no_skip", "skip7", "multires5", "feat255"])
def test_bf16_step_against_emulation(R, name):
    """RNB_VARIANT_BF16 on four fused shapes other than the shipped one, one train step against oracle/bf16_emu.py with
    the rule of tests/test_gpu_bf16_emu.py (feature width 255: the fp32 albedo kernels behind the bf16 SDF sweeps).
    Skip at layer 1, Ep = 32 and feature widths below 225 are refused by make_layout (tests/test_shape_paths.py)."""
    shape = BY_NAME[name]
    assert shape.bf16
    n = bf16_step(R, shape.mc, 64, params=live_params(shape.mc, shape.seed), tag=f"shape {name}")
    assert n == len(O.param_order(shape.mc))
