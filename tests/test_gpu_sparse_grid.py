"""Sparse SDF grid (`rnb_sdf_grid_sparse_*`, `NeuSRenderer.extract_fields_sparse`, `extract_geometry(sparse=True)`) against
the dense grid of the same build, which tests/golden/grid_tiny.npz pins to the reference's extract_fields.

What is asserted, with no tolerance anywhere:
  * samples of evaluated bricks are BIT-EQUAL to `extract_fields(to_host=False)` (same coordinates, same kernel family,
    rows independent of their tile mates);
  * `truth` — the bricks that contain a cell whose 8 dense samples are not all `<= thr` / all `> thr` — is a subset of the
    evaluated bricks (nothing missed), and with `margin = 0` the two sets are equal (nothing evaluated needlessly);
  * samples outside the evaluated bricks are finite, on their brick corners' side of the threshold and within the corners'
    [min, max];
  * marching cubes gives the same arrays on the sparse and on the dense volume.
`truth` always comes from the device's own dense volume."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import mc_oracle as M
from oracle import rnb_oracle as O
from tests.golden_util import Golden
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device

pytestmark = pytest.mark.gpu

LO, HI = torch.tensor([-1.01, -1.01, -1.01]), torch.tensor([1.01, 1.01, 1.01])
GRIDS = [(70, 8, 0.0), (97, 8, 0.0), (193, 8, 0.0), (257, 16, 0.0), (97, 8, 0.05)]   # (resolution, brick, threshold)
MODELS = ["sharp", "geo", "tiny", "sharp_bf16"]


def _params(which):
    if which in ("sharp", "sharp_bf16"):   # trained state, |grad sdf| up to 2.7; fused route (bf16: the bf16 route)
        g = Golden("full_main_sharp")
        return g.mc, g.params()
    if which == "geo":                      # seed-0 geometric init of the full-size network; fused route
        mc = O.ModelConf()
        torch.manual_seed(0)
        return mc, O.init_params(mc)
    assert which == "tiny"                  # the tiny network of tests/test_gpu_edges.py::_tiny (seed 3); per-layer route
    mc = O.ModelConf(sdf=O.SDFConf(d_out=65, d_hidden=64), color=O.ColorConf(d_feature=64, d_hidden=64),
                     render=O.RenderConf(n_samples=16, n_importance=16))
    torch.manual_seed(3)
    p = O.init_params(mc)
    with torch.no_grad():
        p["dev.variance"].fill_(0.4)
    return mc, p


_REN = {}


def _renderer(R, which):
    if which not in _REN:
        mc, p = _params(which)
        ren = R.build_from_named_params(mc, p, device())[3]
        if which == "sharp_bf16":
            ren.set_variant(bf16=True)
        _REN[which] = ren
    return _REN[which]


def _containing(res, bs, nb):
    """per axis: the owner brick of every sample (floor(i / bs), the last brick owns the last layer) and the second brick a
    sample on a low face belongs to (the owner again where there is none)"""
    i = np.arange(res)
    own = np.minimum(i // bs, nb - 1)
    low = np.where((i - own * bs == 0) & (own > 0), own - 1, own)
    return own, low


def _sample_mask(mask, res, bs):
    """bool [res,res,res]: the sample lies in at least one brick of `mask`"""
    nb = mask.shape[0]
    own, low = _containing(res, bs, nb)
    out = np.zeros((res, res, res), dtype=bool)
    for ax in (own, low):
        for ay in (own, low):
            for az in (own, low):
                out |= mask[np.ix_(ax, ay, az)]
    return out


def _truth(u, thr, bs, nb):
    """bool [nb,nb,nb]: the brick contains a cell whose 8 samples are not all inside / all outside (NaN = outside)"""
    ins = u <= thr
    n = ins.shape[0] - 1
    cnt = np.zeros((n, n, n), dtype=np.int8)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                cnt += ins[dx:dx + n, dy:dy + n, dz:dz + n]
    crossed = np.zeros((nb * bs,) * 3, dtype=bool)
    crossed[:n, :n, :n] = (cnt != 0) & (cnt != 8)
    return crossed.reshape(nb, bs, nb, bs, nb, bs).any(axis=(1, 3, 5))


def _check_sparse_against_dense(R, ren, res, bs, thr, margin, ud, u_np):
    us, info = ren.extract_fields_sparse(LO, HI, res, threshold=thr, brick=bs, margin=margin)
    torch.cuda.synchronize()
    geo = R.native.brick_geometry(res, bs)
    nb = geo["nb"]
    mask = info["mask"].cpu().numpy()
    assert mask.shape == (nb, nb, nb) and mask.dtype == bool
    assert info["brick"] == bs and info["bricks_total"] == nb ** 3
    assert info["bricks_active"] == int(mask.sum()) and info["bricks_seeded"] <= info["bricks_active"]
    assert info["points_evaluated"] == (nb + 1) ** 3 + info["bricks_active"] * (bs + 1) ** 3
    truth = _truth(u_np, thr, bs, nb)
    share = info["bricks_active"] / info["bricks_total"]
    print(f"res {res} brick {bs} thr {thr} margin {margin}: seeded {info['bricks_seeded']} active {info['bricks_active']} "
          f"of {info['bricks_total']} ({100 * share:.1f} %), truth {int(truth.sum())}, rounds {info['rounds']}")
    missed = truth & ~mask
    assert not missed.any(), f"crossed bricks left out (an unseeded component?) at {np.argwhere(missed)[:8].tolist()}"
    if margin == 0:
        extra = mask & ~truth
        assert not extra.any(), f"bricks evaluated without a crossed cell at {np.argwhere(extra)[:8].tolist()}"
    assert info["bricks_active"] < info["bricks_total"] / 2, "a sparse call that evaluates (almost) everything"
    # evaluated samples: the dense grid's bits
    act = torch.from_numpy(_sample_mask(mask, res, bs)).to(ud.device)
    assert torch.equal(us[act], ud[act])
    # the others: finite, on their corners' side, inside the corners' range
    us_np = us.cpu().numpy()
    lat = u_np[np.ix_(geo["lattice"], geo["lattice"], geo["lattice"])]
    cmin = np.full((nb, nb, nb), np.inf, dtype=np.float32)
    cmax = np.full((nb, nb, nb), -np.inf, dtype=np.float32)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                c = lat[dx:dx + nb, dy:dy + nb, dz:dz + nb]
                cmin, cmax = np.minimum(cmin, c), np.maximum(cmax, c)
    own = _containing(res, bs, nb)[0]
    smin, smax = cmin[np.ix_(own, own, own)], cmax[np.ix_(own, own, own)]
    off = ~act.cpu().numpy()
    v = us_np[off]
    assert np.isfinite(v).all()
    assert ((v >= smin[off]) & (v <= smax[off])).all()
    assert ((v <= thr) == (smax[off] <= thr)).all() and ((smax[off] <= thr) | (smin[off] > thr)).all()
    # the mesh
    vs, ts = R.marching_cubes(us, thr)
    vd, td = R.marching_cubes(ud, thr)
    torch.cuda.synchronize()
    assert len(td) > 0
    assert np.array_equal(ts.cpu().numpy(), td.cpu().numpy()) and np.array_equal(vs.cpu().numpy(), vd.cpu().numpy())
    return info


@pytest.mark.parametrize("res,bs,thr", GRIDS)
@pytest.mark.parametrize("which", MODELS)
def test_sparse_grid_is_the_dense_grid_near_the_surface(R, which, res, bs, thr):
    ren = _renderer(R, which)
    ud = ren.extract_fields(LO, HI, res, to_host=False)
    u_np = ud.cpu().numpy()
    for margin in (0.0, 1.0):
        info = _check_sparse_against_dense(R, ren, res, bs, thr, margin, ud, u_np)
        if which == "sharp" and (res, bs, thr, margin) == (97, 8, 0.0, 0.0):
            assert info["rounds"] >= 1, "seeds alone miss bricks of this surface: the growth kernel has to run"


@pytest.mark.parametrize("variant", [dict(x2h=False), dict(f32_mfma=True), dict(reg_tile=True)],
                         ids=["six_term", "f32_mfma", "mv_sweep"])
def test_other_arithmetic_variants_of_the_fused_route(R, variant):
    """The six-term and fp32-MFMA forms of the fused sweep and the M/V sweep carry the same brick mode: dense and sparse are
    compared within the variant."""
    mc, p = _params("sharp")
    ren = R.build_from_named_params(mc, p, device())[3]
    ren.set_variant(**variant)
    ud = ren.extract_fields(LO, HI, 97, to_host=False)
    u_np = ud.cpu().numpy()
    for margin in (0.0, 1.0):
        _check_sparse_against_dense(R, ren, 97, 8, 0.0, margin, ud, u_np)


def test_extract_geometry_sparse_equals_dense(R):
    for which, res in (("sharp", 193), ("geo", 96)):
        ren = _renderer(R, which)
        vd, td = ren.extract_geometry(LO, HI, res, threshold=0.0, backend="native")
        vs, ts = ren.extract_geometry(LO, HI, res, threshold=0.0, backend="native", sparse=True)
        assert np.array_equal(ts, td) and np.array_equal(vs, vd)
        info = ren.last_sparse_grid
        assert info["bricks_active"] < info["bricks_total"] / 2 and info["mask"].any()
        # without `sparse` the path is the one it was: extract_fields + marching cubes + rescale
        vo, to = M.marching_cubes(ren.extract_fields(LO, HI, res), 0.0)
        vo = vo / (res - 1.0) * (HI - LO).numpy()[None] + LO.numpy()[None]
        assert np.array_equal(td, to) and np.array_equal(vd, vo)
        if which == "geo":
            V, E, F, euler, closed = M.mesh_report(vs, ts)
            assert closed and euler == 2
    # margin and brick reach the sparse call
    ren = _renderer(R, "geo")
    ren.extract_geometry(LO, HI, 97, backend="native", sparse=True, margin=0.0, brick=16)
    a = ren.last_sparse_grid
    ren.extract_geometry(LO, HI, 97, backend="native", sparse=True, margin=1.0, brick=16)
    assert a["brick"] == 16 and a["bricks_active"] < ren.last_sparse_grid["bricks_active"]


def test_a_margin_that_seeds_every_brick_gives_the_dense_volume(R):
    """The seeding rule itself: with a margin beyond every value of the field each brick is a seed, nothing is left to growth
    or to interpolation, and the volume is the dense one bit for bit."""
    for which, res, bs in (("sharp", 70, 8), ("tiny", 97, 16)):
        ren = _renderer(R, which)
        ud = ren.extract_fields(LO, HI, res, to_host=False)
        us, info = ren.extract_fields_sparse(LO, HI, res, brick=bs, margin=1e6)
        assert info["mask"].all() and info["bricks_seeded"] == info["bricks_total"] == info["bricks_active"]
        assert info["rounds"] == 0
        assert torch.equal(us, ud)


def test_nan_weights_give_an_all_nan_volume_and_an_empty_mesh(R):
    mc, p = _params("geo")
    with torch.no_grad():
        p["sdf.lin0.weight_v"][3, 1] = float("nan")
    ren = R.build_from_named_params(mc, p, device())[3]
    ud = ren.extract_fields(LO, HI, 70, to_host=False)
    assert torch.isnan(ud).all()
    us, info = ren.extract_fields_sparse(LO, HI, 70, brick=8, margin=0.0)
    assert info["mask"].all() and info["bricks_seeded"] == info["bricks_total"]
    assert torch.isnan(us).all()
    v, t = R.marching_cubes(us, 0.0)
    assert v.shape == (0, 3) and t.shape == (0, 3)
    v, t = ren.extract_geometry(LO, HI, 70, backend="native", sparse=True)
    assert v.shape == (0, 3) and t.shape == (0, 3)


def _raw(R, ren, res, bs, margin=1.0, x=None, thr=0.0):
    gd = R.native.GridDesc()
    for d in range(3):
        gd.bound_min[d], gd.bound_max[d] = float(LO[d]), float(HI[d])
    gd.resolution, gd.out_scale = res, -1.0
    gd.x_begin, gd.x_end = x if x is not None else (0, res)
    return gd, R.native.SparseGridDesc(bs, thr, margin)


def test_refusals_leave_the_renderer_usable(R):
    lib = R.native.load()
    ren = _renderer(R, "tiny")
    mc, p = _params("tiny")
    cpu_ren = R.build_from_named_params(mc, p, torch.device("cpu"))[3]
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        cpu_ren.extract_fields_sparse(LO, HI, 33)
    with pytest.raises(ValueError, match="brick"):
        ren.extract_fields_sparse(LO, HI, 33, brick=5)
    with pytest.raises(ValueError, match="margin"):
        ren.extract_fields_sparse(LO, HI, 33, margin=-1.0)
    with pytest.raises(ValueError, match="margin"):
        ren.extract_geometry(LO, HI, 33, backend="native", sparse=True, margin=float("nan"))
    ren.set_data_parallel(group=object())   # (never used: the call refuses before anything collective)
    try:
        with pytest.raises(ValueError, match="data-parallel"):
            ren.extract_fields_sparse(LO, HI, 33)
    finally:
        ren.set_data_parallel(enabled=False)
    # the raw ABI: every refusal comes with RNB_E_INVALID and a message, from the sizing query and from the calls
    packed = ren._pack(False)
    n = torch.full((1,), 77, dtype=torch.int64, device=device())
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=device())
    vol = torch.empty(33, 33, 33, device=device())
    nbytes = C.c_int64()
    bad = [dict(x=(0, 16)), dict(x=(1, 33)), dict(bs=5), dict(bs=0), dict(margin=-1.0), dict(margin=float("nan")),
           dict(res=1)]
    for kw in bad:
        gd, sd = _raw(R, ren, kw.get("res", 33), kw.get("bs", 8), kw.get("margin", 1.0), kw.get("x"))
        with R.native.on_device(device()) as stream:
            rcs = [lib.rnb_sdf_grid_sparse_workspace_bytes(C.byref(ren.desc), C.byref(gd), C.byref(sd), C.byref(nbytes)),
                   lib.rnb_sdf_grid_sparse_seed(C.byref(ren.desc), R.native.ptr(packed), C.byref(gd), C.byref(sd),
                                                R.native.ptr(ws), ws.numel(), R.native.ptr(n), stream),
                   lib.rnb_sdf_grid_sparse_round(C.byref(ren.desc), R.native.ptr(packed), C.byref(gd), C.byref(sd),
                                                 R.native.ptr(vol), R.native.ptr(ws), ws.numel(), 0, 1, R.native.ptr(n),
                                                 stream),
                   lib.rnb_sdf_grid_sparse_finish(C.byref(ren.desc), C.byref(gd), C.byref(sd), R.native.ptr(vol),
                                                  R.native.ptr(ws), ws.numel(), None, stream)]
        assert rcs == [-1, -1, -1, -1], (kw, rcs)          # RNB_E_INVALID
        assert len(lib.rnb_last_error_string()) > 0
    torch.cuda.synchronize()
    assert int(n.item()) == 77, "a refused call launched something"
    # and the renderer still works
    ud = ren.extract_fields(LO, HI, 33, to_host=False)
    us, info = ren.extract_fields_sparse(LO, HI, 33, brick=4, margin=0.0)
    act = torch.from_numpy(_sample_mask(info["mask"].cpu().numpy(), 33, 4)).to(device())
    assert act.any() and torch.equal(us[act], ud[act])


@pytest.mark.parametrize("which", ["tiny", "geo"])
def test_workspace_query_is_honest(R, which):
    """One byte less than the query asks for is refused (RNB_E_WORKSPACE) before any launch; the exact size works."""
    lib = R.native.load()
    ren = _renderer(R, which)
    packed = ren._pack(False)
    gd, sd = _raw(R, ren, 70, 8)
    nbytes = C.c_int64()
    R.native.check(lib.rnb_sdf_grid_sparse_workspace_bytes(C.byref(ren.desc), C.byref(gd), C.byref(sd), C.byref(nbytes)))
    need = nbytes.value
    assert need >= 10 ** 3 * 4 + 9 ** 3 * 5            # lattice + list + one state byte per brick
    ws = torch.empty(need, dtype=torch.uint8, device=device())
    n = torch.full((1,), 77, dtype=torch.int64, device=device())
    vol = torch.empty(70, 70, 70, device=device())
    with R.native.on_device(device()) as stream:
        rc = lib.rnb_sdf_grid_sparse_seed(C.byref(ren.desc), R.native.ptr(packed), C.byref(gd), C.byref(sd),
                                          R.native.ptr(ws), need - 1, R.native.ptr(n), stream)
        assert rc == -2 and b"workspace too small" in lib.rnb_last_error_string()
        rc = lib.rnb_sdf_grid_sparse_round(C.byref(ren.desc), R.native.ptr(packed), C.byref(gd), C.byref(sd),
                                           R.native.ptr(vol), R.native.ptr(ws), need - 1, 0, 1, R.native.ptr(n), stream)
        assert rc == -2
        rc = lib.rnb_sdf_grid_sparse_finish(C.byref(ren.desc), C.byref(gd), C.byref(sd), R.native.ptr(vol),
                                            R.native.ptr(ws), need - 1, None, stream)
        assert rc == -2
        torch.cuda.synchronize()
        assert int(n.item()) == 77, "a refused call launched something"
        R.native.check(lib.rnb_sdf_grid_sparse_seed(C.byref(ren.desc), R.native.ptr(packed), C.byref(gd), C.byref(sd),
                                                    R.native.ptr(ws), need, R.native.ptr(n), stream))
    torch.cuda.synchronize()
    assert 0 < int(n.item()) < 9 ** 3
