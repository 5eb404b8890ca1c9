"""The extraction chain of `extract_geometry` through both backends: `backend="mcubes"` with stages — host marching
cubes, the arrays uploaded, the stages of mesh_pipeline.STAGES on the device — against `backend="native"` with the same
options, BIT FOR BIT.  PyMCubes is not installed where the tests run, so a stand-in module named `mcubes` answers
`marching_cubes(u, threshold)` with the package's own marching cubes: the two backends then differ in nothing but the
route the arrays take, which is what this file checks.  Scene, cameras and masks are those of the renderer's cull test
(tests/test_gpu_mesh_cull.py), which asserts that the cull alone removes something and keeps something."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import mesh_cull_ref as F
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device
from tests.mesh_attrs_util import HI, LO

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RES = 40
_SHARED = {}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device())


def _tiny_renderer(R):
    """the tiny checkpoint's renderer (tests/golden/ref_ckpt_tiny.pth), once"""
    if "ren" not in _SHARED:
        from rnb_neus_fork_amd import checkpoint as CK
        dev = device()
        nc = np.load(os.path.join(GOLDEN, "ref_ckpt_tiny_step3.npz"), allow_pickle=False)["nerf.conf"]
        torch.manual_seed(99)
        nerf = R.NeRF(D=int(nc[0]), W=int(nc[1]), d_in=int(nc[2]), d_in_view=int(nc[3]), multires=int(nc[4]),
                      multires_view=int(nc[5]), output_ch=int(nc[6]), skips=[int(nc[7])], use_viewdirs=True).to(dev)
        sdf = R.SDFNetwork(d_in=3, d_out=65, d_hidden=64, n_layers=8, skip_in=[4], multires=6).to(dev)
        devn = R.SingleVarianceNetwork(0.1).to(dev)
        col = R.RenderingNetwork(d_feature=64, mode="no_view_dir", d_in=6, d_out=3, d_hidden=64, n_layers=2, multires_view=4).to(dev)
        ren = R.NeuSRenderer(nerf, sdf, devn, col, n_samples=16, n_importance=16, n_outside=0, up_sample_steps=4, perturb=1.0)
        params = list(nerf.parameters()) + list(sdf.parameters()) + list(devn.parameters()) + list(col.parameters())
        CK.load_checkpoint(os.path.join(GOLDEN, "ref_ckpt_tiny.pth"), nerf, sdf, devn, col, R.FlatAdam(params, lr=1.0),
                           map_location=dev)
        _SHARED["ren"] = ren
    return _SHARED["ren"]


def _options():
    """clean, the three-camera cull of test_the_renderer_cull_keyword (left half of every mask cut away), simplify"""
    s = F.scene()
    masks = s["masks"][:3].copy()
    masks[:, :, :24] = 0
    cull = dict(projections=_dev(s["projections"][:3]), eyes=_dev(s["eyes"][:3]), masks=_dev(masks * np.uint8(255)),
                max_outside=1)
    return {"clean": {"keep_largest": 1}, "cull": cull, "simplify": {"cell_size": 2.0}}


def _stand_in(R, calls):
    """a module that answers `mcubes.marching_cubes(u, threshold)` as PyMCubes does — numpy in, numpy out — with the
    package's marching cubes"""
    stub = types.ModuleType("mcubes")

    def marching_cubes(u, threshold):
        assert isinstance(u, np.ndarray) and u.shape == (RES, RES, RES), "the mcubes backend hands over the host volume"
        calls.append(float(threshold))
        v, t = R.marching_cubes(torch.from_numpy(u).to(device()), threshold)
        return v.cpu().numpy(), t.cpu().numpy()

    stub.marching_cubes = marching_cubes
    return stub


def _infos(ren):
    return {k: getattr(ren, k) for k in ("last_mesh_clean", "last_mesh_cull", "last_mesh_simplify")}


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("staged", [True, False], ids=["stages", "plain"])
def test_the_mcubes_backend_runs_the_chain_of_the_native_one(R, monkeypatch, staged, sparse):
    ren = _tiny_renderer(R)
    options = _options() if staged else {}
    plain_t = ren.extract_geometry(LO, HI, RES, threshold=0.0, backend="native", sparse=sparse)[1]
    assert len(plain_t) > 500
    want_v, want_t = ren.extract_geometry(LO, HI, RES, threshold=0.0, backend="native", sparse=sparse, **options)
    assert ren.last_mesh_backend == "native"
    want_info, want_grid = _infos(ren), ren.last_sparse_grid
    if staged:      # the three stages together remove something and keep something, and each of them ran
        assert 0 < len(want_t) < len(plain_t)
        n = [want_info[k]["n_triangles"] for k in ("last_mesh_clean", "last_mesh_cull", "last_mesh_simplify")]
        assert n[0][0] == len(plain_t) and n[0][1] == n[1][0] and n[1][1] == n[2][0] and n[2][1] == len(want_t)
        for k in want_info:
            setattr(ren, k, None)
    calls = []
    monkeypatch.setitem(sys.modules, "mcubes", _stand_in(R, calls))
    got_v, got_t = ren.extract_geometry(LO, HI, RES, threshold=0.0, backend="mcubes", sparse=sparse, **options)
    assert calls == [0.0] and ren.last_mesh_backend == "mcubes"
    assert got_v.dtype == np.float64 and got_v.shape == want_v.shape and got_t.dtype == np.int32
    assert np.array_equal(got_v.view(np.uint64), want_v.view(np.uint64)), "vertices differ between the backends"
    assert np.array_equal(got_t, want_t), "triangles differ between the backends"
    if staged:
        for k, info in _infos(ren).items():
            assert info["n_vertices"] == want_info[k]["n_vertices"] and info["n_triangles"] == want_info[k]["n_triangles"], k
    if sparse:
        grid = ren.last_sparse_grid
        assert grid is not want_grid and all(grid[k] == want_grid[k] for k in ("brick", "bricks_seeded", "bricks_active", "rounds"))
        assert torch.equal(grid["mask"], want_grid["mask"])
