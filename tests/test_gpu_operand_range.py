"""x2h operand range: outliers where the FIRST rescale vote of a tile has to find them.

The default arithmetic ("x2h", include/rnbneus.h) holds an operand tile in LDS times a power of two: 2^6 while every value of
the tile stays below kH2ActLimit = 256, else a scale from the tile's own maximum.  Three votes decide that for the first tile
of a sweep: the network input of the forward sweeps (fused.hip, also rnb_sdf_grid), the seed w_sdf * D of the reverse sweep
(fused_bwd.hip) and the points / normals entering the albedo network (color_h2.hip).  Through round 5 each ballot ran inside
`if (lane == 0)` and saw one lane per wave: row 0 of the tile (forward, albedo) or columns 0..3 of the seed (reverse).  An
outlier anywhere else kept the fixed scale, and beyond 65520 / 2^6 = 1023.75 the fp16 hi plane overflowed to inf.

Every case below asserts on the host that its outlier sits where such a vote does not look, at both tile heights the sweeps
use (64 rows: TI=2; 32 rows: TI=1, small batches and the sampling forwards), and holds the device to the fp64 oracle with the
calibration of tests/parity.py, per row group:
    in-range rows   the output rule (parity.check_value) with its factor K_OUT                         (over those rows only;
                    this includes the outlier's neighbours, which now run at their tile's smaller scale)
    outlier rows    the same with factor 10 (sin(2^5 x) of x ~ 1e3 is ill-conditioned in ANY fp32, as in
                    test_x2h_has_no_operand_range's coordinates of 3000)"""
import math

import pytest
import torch

from oracle import rnb_oracle as O
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device, step_against_fp64
from tests.parity import K_OUT, check_value, value_errors

pytestmark = pytest.mark.gpu

LIMIT = 256.0              # kH2ActLimit: a tile holding a value at or beyond it must leave the fixed scale
OLD_HI = 65520.0 / 64.0    # beyond this the fixed scale 2^6 rounds the fp16 hi plane to inf
K_ILL = 10.0               # the outlier's own rows (ill-conditioned in any fp32; the existing factor of the range test)
TILE_HEIGHTS = (32, 64)


def _tiles(v, T):
    """[N, ...] -> [tiles, T, ...], zero padded (the device pads a ragged batch with zero rows)"""
    pad = (-v.shape[0]) % T
    if pad:
        v = torch.cat([v, v.new_zeros((pad,) + tuple(v.shape[1:]))])
    return v.reshape(-1, T, *v.shape[1:])


def _row0_vote_misses(rowmax, T):
    """Some T-row tile has row 0 below the limit and another row beyond the old hi-plane limit: a tile that a vote looking
    at row 0 alone waves through at the fixed scale."""
    t = _tiles(rowmax, T)
    return bool(((t[:, 0] < LIMIT) & (t[:, 1:].amax(dim=1) > OLD_HI)).any())


def _seed_vote_misses(seed, T):
    """Some T-row tile of the reverse sweep's seed has columns 0..3 (what lane 0 holds) below the limit and another column
    beyond the old hi-plane limit."""
    t = _tiles(seed.abs(), T)
    return bool(((t[:, :, :4].amax(dim=(1, 2)) < LIMIT) & (t.amax(dim=(1, 2)) > OLD_HI)).any())


def _named_sdf(sdf, dt):
    return {("sdf." + n): q.detach().cpu().to(dt) for n, q in sdf.named_parameters()}


def _oracle(named, conf, pts, dt):
    """(sdf [N,1], d sdf / dx [N,3]) of the oracle in dtype dt"""
    p = {k: v.to(dt) for k, v in named.items()}
    x = pts.detach().cpu().to(dt).requires_grad_(True)
    with torch.enable_grad():
        y = O.sdf_forward(p, conf, x)[:, :1]
        (n,) = torch.autograd.grad(y.sum(), x)
    return y.detach(), n.detach()


def _seed(named, conf, pts):
    """w_sdf * D_last per point and column (fp64): the seed of the reverse sweep"""
    p = {k: v.double() for k, v in named.items()}
    inputs = O.embed(pts.detach().cpu().double() * conf.scale, conf.multires)
    x = inputs
    n_lin = conf.n_layers + 1
    for l in range(n_lin - 1):
        if l in conf.skip_in:
            x = torch.cat([x, inputs], dim=1) / math.sqrt(2.0)
        pre = torch.nn.functional.linear(x, O.effective_weight(p, f"sdf.lin{l}"), p[f"sdf.lin{l}.bias"])
        x = O.softplus100(pre)
    d_last = torch.sigmoid(100.0 * pre)
    return O.effective_weight(p, f"sdf.lin{n_lin - 1}")[0] * d_last


def _check_rows(tag, what, got, ref64, ref32, ill):
    """the calibrated bound per row group (module docstring); `ill`: bool [N], the outlier rows.  Returns
    {group: e_hip / e_ref32}."""
    got = got.detach().cpu().double().reshape(ref64.shape)
    assert bool(torch.isfinite(got).all()), f"{tag}: {what}: not finite at rows {(~torch.isfinite(got)).any(-1).nonzero()[:8].flatten().tolist()}"
    ratios = {}
    for group, rows, k in (("in-range", ~ill, K_OUT), ("outlier", ill, K_ILL)):
        if not bool(rows.any()):
            continue
        e_hip, e_ref, _ = value_errors(got[rows], ref64[rows], ref32[rows], k=k)
        ratios[group] = e_hip / max(e_ref, 1e-30)     # (printed as a multiple of the fp32 oracle's error, not of the bound)
        check_value(f"{tag}: {what}, {group} rows (factor {k})", got[rows], ref64[rows], ref32[rows], k=k)
    return ratios


def _points_desc(R, sdf, ti, x2h):
    """descriptor + packed weights of a point-wise query with the tile height forced (ti = 1: 32 rows, 2: 64 rows; None:
    the library's choice) and the arithmetic chosen (x2h=False: six bf16 terms, which have their range by construction)"""
    desc = R.runtime.model_desc(sdf, None)
    desc.variant = R.native.variant_bits(fwd_ti=ti or 0, bwd_ti=ti or 0, x2h=None if x2h else False)
    return desc, R.runtime.pack_weights(desc, sdf, None, device())


@torch.no_grad()
def _query(R, sdf, pts, ti, x2h=True):
    """(sdf, normal) of the device.  ti=None with x2h: the public SDFNetwork.sdf / .gradient"""
    pts = pts.to(device())
    if ti is None:
        assert x2h
        return sdf.sdf(pts), sdf.gradient(pts).reshape(-1, 3)
    desc, packed = _points_desc(R, sdf, ti, x2h)
    return R.runtime.sdf_forward(desc, packed, pts, False), R.runtime.sdf_gradient(desc, packed, pts)


@pytest.fixture(scope="module")
def net(R):
    """the full-size network (O.ModelConf(), 256 wide), 4096 + 37 points in [-1, 1]^3 and their oracle values"""
    mc = O.ModelConf()
    torch.manual_seed(6)
    p = O.init_params(mc)
    sdf, devn, col, ren = R.build_from_named_params(mc, p, device())
    gen = torch.Generator().manual_seed(2)
    pts = torch.rand(4096 + 37, 3, generator=gen) * 2 - 1
    torch.set_num_threads(16)
    named = _named_sdf(sdf, torch.float32)
    r64, r32 = _oracle(named, mc.sdf, pts, torch.float64), _oracle(named, mc.sdf, pts, torch.float32)
    return dict(mc=mc, p=p, sdf=sdf, ren=ren, pts=pts, named=named, r64=r64, r32=r32)


# ---------------------------------------------------------------------------------------------------------------------------
# A. one point-wise input outlier off row 0 (sweep F, and through the saved state sweep R)
# ---------------------------------------------------------------------------------------------------------------------------
TILE = 5   # the 64-row tile that holds the outlier


def _outlier_case(net, n, row, M):
    """the first n points with coordinate (row % 3) of `row` set to +-M; oracle values with that row replaced"""
    pts = net["pts"][:n].clone()
    pts[row, row % 3] = M if row % 2 else -M
    one = {dt: _oracle(net["named"], net["mc"].sdf, pts[row:row + 1], dt) for dt in (torch.float64, torch.float32)}
    refs = []
    for dt, base in ((torch.float64, net["r64"]), (torch.float32, net["r32"])):
        y, g = base[0][:n].clone(), base[1][:n].clone()
        y[row], g[row] = one[dt][0][0], one[dt][1][0]
        refs.append((y, g))
    rowmax = pts.abs().amax(dim=1) * net["mc"].sdf.scale
    return pts, refs, rowmax >= LIMIT, rowmax


def _run_outlier(R, net, tag, pts, refs, ill, ti, x2h):
    (y64, g64), (y32, g32) = refs
    y, g = _query(R, net["sdf"], pts, ti, x2h)
    ry = _check_rows(tag, "sdf", y, y64, y32, ill)
    rg = _check_rows(tag, "normal", g, g64, g32, ill)
    print(f"OPRANGE {tag}: hip / fp32-oracle error ratio, in-range rows: sdf {ry['in-range']:.2f}, normal "
          f"{rg['in-range']:.2f} (bound {K_OUT}); outlier row: sdf {ry['outlier']:.2f}, normal {rg['outlier']:.2f} (bound {K_ILL})")


@pytest.mark.parametrize("x2h", [True, False], ids=["x2h", "bf16x6"])
@pytest.mark.parametrize("ti", [1, 2], ids=["tile32", "tile64"])
@pytest.mark.parametrize("M", [1100.0, 3000.0])
@pytest.mark.parametrize("pos", [1, 17, 31, 45, 63, 0, 32])
def test_input_outlier_off_row_0(R, net, pos, M, ti, x2h):
    """4096 points, one of them with a coordinate of +-M on row `pos` of a 64-row tile: sdf and normal against fp64.  Rows 0
    and 32 are the controls (row 0 of a tile at both heights / at the 32-row height): there even the old vote saw it."""
    row = TILE * 64 + pos
    pts, refs, ill, rowmax = _outlier_case(net, 4096, row, M)
    assert int(ill.sum()) == 1 and bool(ill[row]) and float(rowmax[row]) > OLD_HI
    for T in TILE_HEIGHTS:   # the construction itself: off row 0 where promised, on row 0 for the controls
        assert _row0_vote_misses(rowmax, T) == (pos % T != 0), f"row {pos} at tile height {T}: the construction drifted"
    _run_outlier(R, net, f"input outlier {M:g} on row {pos}, {32 * ti}-row tiles, {'x2h' if x2h else 'bf16 x6'}",
                 pts, refs, ill, ti, x2h)


@pytest.mark.parametrize("ti,x2h", [(None, True), (1, True), (2, True), (1, False), (2, False)],
                         ids=["default", "tile32", "tile64", "tile32-bf16x6", "tile64-bf16x6"])
@pytest.mark.parametrize("M", [1100.0, 3000.0])
def test_input_outlier_on_the_last_row_of_a_ragged_batch(R, net, M, ti, x2h):
    """N = 4096 + 37: the outlier on the last valid row of the partial last tile (the rows behind it are padding)"""
    n = 4096 + 37
    pts, refs, ill, rowmax = _outlier_case(net, n, n - 1, M)
    for T in TILE_HEIGHTS:
        assert (n - 1) % T != 0 and _row0_vote_misses(rowmax, T), f"tile height {T}: the construction drifted"
    _run_outlier(R, net, f"ragged N={n}, outlier {M:g} on the last row, ti={ti}, {'x2h' if x2h else 'bf16 x6'}",
                 pts, refs, ill, ti, x2h)


def test_variant_switch_reaches_the_point_entry_points(R, net):
    """The bf16 x6 control above is only a control if the descriptor's variant bits reach rnb_sdf_forward /
    rnb_sdf_gradient: the two arithmetics must round differently somewhere on 4096 in-range points.  (SDFNetwork.sdf /
    .gradient build a descriptor of their own, so NeuSRenderer.set_variant does not reach them; the cases above pass the
    variant in the descriptor of the point-wise calls.)"""
    pts = net["pts"][:4096]
    a, b = _query(R, net["sdf"], pts, 2, True), _query(R, net["sdf"], pts, 2, False)
    assert not (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])), "x2h=False changed nothing: the switch does not arrive"


# ---------------------------------------------------------------------------------------------------------------------------
# B. the reverse sweep's seed: one column of w_sdf (row 0 of lin8) pushed to 3e4
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", [2, 4, 130, 255])
def test_reverse_seed_column_pushed(R, net, j):
    """w_sdf[j] = 3e4, the other columns unchanged (v := w_new, g := |w_new|): the seed gz = w_sdf * D_last is ~1e4 in column
    j of every row.  Column 2 is the control (lane 0 holds columns 0..3).  4096 in-range points, sdf and normal vs fp64, at
    both tile heights of the reverse sweep."""
    mc = net["mc"]
    p = {k: v.clone() for k, v in net["p"].items()}
    w = O.effective_weight(p, "sdf.lin8")[0].clone()
    w[j] = 3.0e4
    p["sdf.lin8.weight_v"][0] = w
    p["sdf.lin8.weight_g"][0] = w.norm()
    sdf, devn, col, ren = R.build_from_named_params(mc, p, device())
    pts = net["pts"][:4096]
    named = _named_sdf(sdf, torch.float32)
    seed = _seed(named, mc.sdf, pts)
    assert float(seed[:, j].abs().max()) > OLD_HI
    for T in TILE_HEIGHTS:
        assert _seed_vote_misses(seed, T) == (j >= 4), f"column {j} at tile height {T}: the construction drifted"
    (y64, g64), (y32, g32) = _oracle(named, mc.sdf, pts, torch.float64), _oracle(named, mc.sdf, pts, torch.float32)
    ill = torch.zeros(pts.shape[0], dtype=torch.bool)
    for ti in (1, 2):
        tag = f"w_sdf[{j}] = 3e4, {32 * ti}-row tiles"
        y, g = _query(R, sdf, pts, ti)
        ry = _check_rows(tag, "sdf", y, y64, y32, ill)
        rg = _check_rows(tag, "normal", g, g64, g32, ill)
        print(f"OPRANGE {tag}: hip / fp32-oracle error ratio: sdf {ry['in-range']:.2f}, normal {rg['in-range']:.2f} (bound {K_OUT})")


# ---------------------------------------------------------------------------------------------------------------------------
# C. the grid path: coordinates generated inside the forward kernel (rnb_sdf_grid)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid(net):
    """x, y in [-1, 1], z in [0, 3000] at resolution 64: a tile is one z-line; its row 0 is z = 0 and its rows past z ~ 1023
    lie in the first 32 rows as well as in the 64"""
    res = 64
    lo, hi = torch.tensor([-1.0, -1.0, 0.0]), torch.tensor([1.0, 1.0, 3000.0])
    xs = [torch.linspace(float(lo[i]), float(hi[i]), res) for i in range(3)]
    xx, yy, zz = torch.meshgrid(*xs, indexing="ij")
    pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], dim=-1)
    named = net["named"]
    with torch.no_grad():
        r64 = -O.sdf_forward({k: v.double() for k, v in named.items()}, net["mc"].sdf, pts.double())[:, :1]
        r32 = -O.sdf_forward(named, net["mc"].sdf, pts)[:, :1]
    return dict(res=res, lo=lo, hi=hi, pts=pts, r64=r64, r32=r32)


@pytest.mark.parametrize("ti", [0, 1], ids=["default-tile64", "tile32"])
def test_grid_with_far_coordinates(R, net, grid, ti):
    rowmax = grid["pts"].abs().amax(dim=1) * net["mc"].sdf.scale
    for T in TILE_HEIGHTS:
        assert _row0_vote_misses(rowmax, T), f"tile height {T}: the construction drifted"
    ren = net["ren"]
    ren.set_variant(fwd_ti=ti)
    try:
        u = ren.extract_fields(grid["lo"], grid["hi"], grid["res"], to_host=False)
    finally:
        ren.set_variant()
    res = grid["res"]
    assert tuple(u.shape) == (res, res, res)
    tag = f"grid z in [0, 3000], {'64' if ti != 1 else '32'}-row tiles"
    r = _check_rows(tag, "volume", u.reshape(-1, 1), grid["r64"], grid["r32"], rowmax >= LIMIT)
    print(f"OPRANGE {tag}: hip / fp32-oracle error ratio, in-range rows {r['in-range']:.2f} (bound {K_OUT}), "
          f"rows beyond {LIMIT:g} {r['outlier']:.2f} (bound {K_ILL})")


# ---------------------------------------------------------------------------------------------------------------------------
# D. train steps: F(save), the albedo forward, every backward kernel and the weight gradients
# ---------------------------------------------------------------------------------------------------------------------------
FAR_RAYS = list(range(0, 64, 8))
KEEP = 70


def _train_setup(R, p=None):
    mc = O.ModelConf()
    if p is None:
        torch.manual_seed(6)
        p = O.init_params(mc)
    sdf, dev, col, ren = R.build_from_named_params(mc, p, device())
    return mc, p, sdf, dev, col, ren, O.synthetic_batch(64, seed=41, step=3, warmup=False)


@torch.no_grad()
def _sampled_z(ren, batch):
    b = {k: v.to(device()) for k, v in batch.items()}
    ren.render_rnb(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=1.0, t_rand=b["t_rand"])
    return ren.last_z_vals.detach().cpu().clone()


@pytest.mark.parametrize("ti", [0, 2], ids=["default-tile32", "tile64"])
def test_train_step_with_far_samples(R, ti):
    """The device's own depths of a 64-ray step; on 8 rays the first 70 samples are kept and the last 58 moved so far out that
    their points have a coordinate in [1030, 1100] (depth (c + |o|) / max|d_i|; the depth itself is larger).  Sample 64 of
    those rays is row 0 of a tile at both heights and in range; the rows behind it are far beyond 1023.  Outputs
    and all 37 parameter gradients against fp64 at the calibrated bounds."""
    mc, p, sdf, dev, col, ren, batch = _train_setup(R)
    z = _sampled_z(ren, batch)
    S = z.shape[1]
    assert S == 128
    o, d = batch["rays_o"], batch["rays_d"]
    for r in FAR_RAYS:
        c = torch.linspace(1030.0, 1100.0, S - KEEP, dtype=torch.float64)
        z[r, KEEP:] = ((c + float(o[r].norm())) / float(d[r].abs().max())).float()
    assert bool((z[:, 1:] >= z[:, :-1]).all())
    rowmax = (o[:, None, :] + d[:, None, :] * z[..., None]).abs().amax(-1) * mc.sdf.scale
    assert float(rowmax[FAR_RAYS, KEEP:].min()) > 1030.0 - 1e-3 and float(rowmax[:, :KEEP].max()) < LIMIT
    for T in TILE_HEIGHTS:
        assert _row0_vote_misses(rowmax.reshape(-1), T), f"tile height {T}: the construction drifted"
    if ti:
        ren.set_variant(fwd_ti=ti)
    ren.track_range = True
    out = step_against_fp64(R, mc, p, sdf, dev, col, ren, batch, f"far samples, fwd_ti={ti}", survey=False, z_vals=z)
    rep = ren.range_report()
    ren.track_range = False
    print(f"OPRANGE far samples, fwd_ti={ti}: " + ", ".join(f"{k} {v:.4g}" for k, v in rep.items()))
    assert rep["max_abs_activation"] > 1023.0
    del out


@pytest.mark.parametrize("j", [4, 130])
def test_train_step_with_pushed_sdf_column(R, j):
    """Unit j of lin7 made constant (weight_g[j] tiny, bias[j] = 0: a_j = ln2 / 100, D_j = 1/2), w_sdf[j] = 3e4 and
    3e4 ln2 / 100 taken off lin8.bias[0], so the surface stays: the reverse sweep's seed is ~1.5e4 in column j of every
    row.  One train step on the sampled depths, outputs and all 37 parameter gradients against fp64."""
    mc = O.ModelConf()
    torch.manual_seed(6)
    p = O.init_params(mc)
    w = O.effective_weight(p, "sdf.lin8")[0].clone()
    w[j] = 3.0e4
    with torch.no_grad():
        p["sdf.lin7.weight_g"][j] = 1e-6
        p["sdf.lin7.bias"][j] = 0.0
        p["sdf.lin8.weight_v"][0] = w
        p["sdf.lin8.weight_g"][0] = w.norm()
        p["sdf.lin8.bias"][0] -= 3.0e4 * math.log(2.0) / 100.0
    mc, p, sdf, dev, col, ren, batch = _train_setup(R, p)
    z = _sampled_z(ren, batch)
    pts = (batch["rays_o"][:, None, :] + batch["rays_d"][:, None, :] * z[..., None]).reshape(-1, 3)
    seed = _seed(_named_sdf(sdf, torch.float32), mc.sdf, pts)
    assert float(seed[:, j].abs().min()) > 1.4e4
    for T in TILE_HEIGHTS:
        assert _seed_vote_misses(seed, T), f"tile height {T}: the construction drifted"
    ren.track_range = True
    out = step_against_fp64(R, mc, p, sdf, dev, col, ren, batch, f"w_sdf[{j}] = 3e4", survey=False, z_vals=z)
    rep = ren.range_report()
    ren.track_range = False
    print(f"OPRANGE w_sdf[{j}] = 3e4 step: " + ", ".join(f"{k} {v:.4g}" for k, v in rep.items()))
    assert rep["max_abs_jacobian_row"] > 1023.0
    del out
