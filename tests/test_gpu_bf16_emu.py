"""RNB_VARIANT_BF16 (csrc/bf16_*.hip) against the bf16-emulating statement (oracle/bf16_emu.py): the same roundings at
the same sites on the device's own fp32 weights, so device and emulation differ only by summation order and the rare
bf16 rounding that order flips.  tests/test_gpu_bf16.py stays as the coarse check against the fp32 oracle.

Bound rule (its constants and the step itself are tests/bf16_emu_step.py), the form of `step_against_fp64` in
tests/gpu_support.py, per output tensor (rms over points) and per
gradient tensor (rel-L2):

    err(device, emu64) <= min(K * max_i err(emu32_i, emu64) + FLOOR, CAP)

emu64: the emulation with fp64 products and sums; emu32_i: the same roundings in fp32, i = one matrix product per
weight gradient ("mm") and 64-point tiles summed in sequence ("tiles").  K = 4; FLOOR = 5e-5 (outputs, rms), 2e-5 (the
loss, relative), 1e-4 (gradients, rel-L2).  The rms floor covers the small cases whose rms is one flipped rounding (65
points: device 6.0e-5 against emu32 1.3e-5; 37 x 24 points, `weights`: 4.0e-5 against 7.9e-6).  CAP is 1/10 of
tests/test_gpu_bf16.py's bound for the same quantity: SDF 1e-3, features 3e-3, normals 1e-2, render outputs 3e-3, loss
2e-3 relative, gradients 1.5e-2 rel-L2.

The max-abs error of a point-wise output is not a summation-order statistic: it is set by the one point where a rounding
decision flipped early in the chain, and emu32 and emu64 (the same arithmetic in another order) already differ by up to
3e-3 in the SDF at 5,000-65,573 points and 7.7e-3 in cdf_fine at 512 x 64 points (measured on MI355X).  Max-abs is
therefore held to 1/2 of tests/test_gpu_bf16.py's bound, without calibration; the rms is the binding check.
Measured on MI355X: err(device) / max_i err(emu32_i) <= 2.1 for every gradient tensor of every step and <= 2.3 for
every output rms with more than a few hundred points.  Every ratio is printed (`pytest -s`)."""
import ctypes as C

import pytest
import torch

from oracle import rnb_oracle as O
from oracle.bf16_emu import Bf16FinePass, bf16_color_supported, mirror_matrices, packed_layout, unfragment, \
    weights_from_packed
from tests.bf16_emu_step import MODES, OLD, Check, linspace_at, model, packed_weights, step
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- 1
def test_bf16_weight_mirror_is_exact(R):
    """The bf16 mirror rnb_weightnorm_fwd appends to `packed` is rb(fp32 weights) bit for bit, every matrix (SDF hidden
    layers and their transposes, the feature head, the albedo hidden layers), after undoing the fragment order."""
    mc = O.ModelConf()
    p, sdf, dev, col, ren = model(R, mc, seed=9)
    packed, total = packed_weights(ren, mc)
    mirror = packed[total:].view(torch.int16)
    mats = mirror_matrices(mc)
    assert len(mats) == 2 * (mc.sdf.n_layers + 1 + mc.color.n_layers)
    for name, off, N, K_ in mats:
        w = packed[off:off + N * K_].reshape(N, K_)
        got = unfragment(mirror[off:off + N * K_], N, K_)
        assert torch.equal(got.view(torch.int32), w.to(torch.bfloat16).to(torch.float32).view(torch.int32)), name
    # the skip layer's W really is the folded one (the emulation relies on it)
    e = packed_layout(mc)["hid"][mc.sdf.skip_in[0]]
    w = packed[e["w"]:e["w"] + e["Np"] * e["Kp"]].reshape(e["Np"], e["Kp"])[:, :e["K"]].double()
    v, g = p["sdf.lin4.weight_v"].double(), p["sdf.lin4.weight_g"].double()
    torch.testing.assert_close(w, v * (g / v.norm(dim=1, keepdim=True)) * 0.5 ** 0.5, rtol=2e-7, atol=1e-9)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("n,ti,sharpen", [(1, 2, False), (63, 1, True), (65, 2, True), (5000, 1, False),
                                          (5000, 2, True), (65536 + 37, 2, False), (65536 + 37, 1, True)])
def test_bf16_pointwise_sdf_and_normal_vs_emulation(R, n, ti, sharpen):
    mc = O.ModelConf()
    p, sdf, dev, col, ren = model(R, mc, seed=1, sharpen=sharpen, fwd_ti=ti, bwd_ti=ti)
    from rnb_neus_fork_amd import runtime
    g = torch.Generator().manual_seed(n)
    pts = (torch.rand(n, 3, generator=g) * 2 - 1) * 0.9
    packed, total = packed_weights(ren, mc)
    pk = packed.to(device())
    out = runtime.sdf_forward(ren.desc, pk, pts.to(device()), True).cpu()
    nrm = runtime.sdf_gradient(ren.desc, pk, pts.to(device())).cpu()
    w = weights_from_packed(packed[:total], mc)
    res = []
    for dt, order in ((torch.float64, "mm"),) + MODES:
        fp = Bf16FinePass(p, mc, w, dtype=dt, order=order)
        s_, f_, n_ = fp.forward_points(pts, use_color=False)
        res.append((s_.double(), fp.feat_fp32.double(), n_.double()))
    ref = res[0]
    chk = Check(f"pointwise n={n} ti={ti} sharpen={sharpen}")
    for i, (name, d) in enumerate((("sdf", out[:, :1]), ("feature", out[:, 1:]), ("normal", nrm))):
        chk.output(name, d, ref[i], [r[i] for r in res[1:]], OLD[name])
    chk.finish()


# ---------------------------------------------------------------------------------------------------------------- 3, 4
CONF5 = O.RenderConf(n_samples=128, n_importance=128, up_sample_steps=4)
RAGGED = O.RenderConf(n_samples=16, n_importance=8, up_sample_steps=4)     # S = 24


@pytest.mark.parametrize("api,no_albedo", [("render_rnb", False), ("render_rnb_warmup", False), ("render_rnb", True),
                                           ("render", False)])
def test_bf16_step_config5_vs_emulation(R, api, no_albedo):
    """BASELINE config 5's shape (48 rays x (128 + 128) samples), every output, the loss and every gradient."""
    n = step(R, O.ModelConf(render=CONF5), 48, api, no_albedo)
    assert n >= (19 if no_albedo else 25)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("B", [1, 3, 37])
def test_bf16_step_ragged_vs_emulation(R, B, det):
    """B x 24 points: never a multiple of the 64-point tiles (the partial last tile of every sweep and dW job)."""
    step(R, O.ModelConf(render=RAGGED), B, deterministic=det)


def test_bf16_step_deterministic_config5_vs_emulation(R):
    step(R, O.ModelConf(render=CONF5), 48, deterministic=True)


def test_bf16_step_b512_vs_emulation(R):
    step(R, O.ModelConf(render=O.RenderConf(n_samples=32, n_importance=32, up_sample_steps=4)), 512)


@pytest.mark.parametrize("n_layers,multires_view,bf16_albedo", [(3, 4, True), (2, 6, False)])
def test_bf16_albedo_shapes_vs_emulation(R, n_layers, multires_view, bf16_albedo):
    """Three hidden albedo layers (still the bf16 albedo kernels), and multires_view = 6: 334 input columns, padded to
    352 > CMAX = 320, the fp32 albedo path behind the bf16 SDF sweeps."""
    mc = O.ModelConf(color=O.ColorConf(n_layers=n_layers, multires_view=multires_view), render=RAGGED)
    assert bf16_color_supported(mc) == bf16_albedo
    L = packed_layout(mc)
    assert (L["Cinp"] <= 320) == bf16_albedo
    n = step(R, mc, 37, sharpen=False, seed=7, tag=f"albedo n_layers={n_layers} multires_view={multires_view}")
    assert n == 3 * (mc.sdf.n_layers + 1) + 1 + 3 * (n_layers + 1)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_bf16_sdf_grid_vs_emulation(R):
    """rnb_sdf_grid under the bf16 variant (api.hip:213): odd resolution 70, an x-slab subset, the bounds of
    tests/test_gpu_edges.py, against the emulation on the grid coordinates the kernel generates."""
    mc = O.ModelConf()
    p, sdf, dev, col, ren = model(R, mc, seed=3, sharpen=True)
    lib = R.native.load()
    res, x0, x1 = 70, 23, 51
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
    vol = vol.cpu()
    assert bool(torch.isfinite(vol).all())
    xs = [linspace_at(lo[0], hi[0], res, torch.arange(x0, x1)), linspace_at(lo[1], hi[1], res, torch.arange(res)),
          linspace_at(lo[2], hi[2], res, torch.arange(res))]
    xx, yy, zz = torch.meshgrid(*xs, indexing="ij")
    pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], dim=-1)
    pk = packed.cpu()
    total = packed_layout(mc)["total"]
    w = weights_from_packed(pk[:total], mc)
    res_ = []
    for dt, order in ((torch.float64, "mm"),) + MODES:
        fp = Bf16FinePass(p, mc, w, dtype=dt, order=order)
        res_.append(-fp.forward_points(pts, use_color=False)[0].double().reshape(vol.shape))
    chk = Check(f"sdf_grid res={res} x={x0}..{x1}")
    chk.output("sdf", vol, res_[0], res_[1:], OLD["sdf"])
    chk.finish()
