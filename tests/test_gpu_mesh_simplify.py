"""Mesh simplification on the device (csrc/mesh_simplify.hip through `simplify_mesh` and the renderer's `simplify=`)
against the numpy reference of tests/mesh_simplify_ref.py.

Every output is an integer or a copy of an input coordinate with a canonical definition, so every comparison is
`array_equal` (`equal_nan` where coordinates are compared) and two runs are bit-equal.  The one geometric bound is derived:
a surviving triangle is the image of an input triangle whose corners each moved within one cell, so every point of the
output lies within sqrt(3) h of the input surface.  References are computed once per mesh and grid and shared."""
import math
import os

import numpy as np
import pytest
import torch

from tests import mesh_components_ref as F
from tests import mesh_simplify_ref as S
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device
from tests.mc_shapes import sphere

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_MC = {}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device())


def _np(x):
    return x.cpu().numpy()


def _arrays(v, t):
    return np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3)


def _check(R, v, t, h, origin=None, ref=None, tag="", twice=False):
    """simplify_mesh against the reference: every output, every count; returns (device result, reference)"""
    v, t = _arrays(v, t)
    want = S.simplify(v, t, h, origin) if ref is None else ref
    attrs = {"id": _dev(np.arange(len(v), dtype=np.float32)), "pair": _dev(np.stack([v[:, 0], -v[:, 2]], axis=1))}
    kw = {} if origin is None else {"origin": tuple(float(x) for x in origin)}
    got = R.simplify_mesh(_dev(v), _dev(t), cell_size=h, attributes=attrs, **kw)
    info = got["info"]
    counts = [info["n_vertices"][1], info["n_triangles"][1], info["n_degenerate"], info["n_duplicate"],
              int(info["skipped"]["bad_index"]) | 2 * int(info["skipped"]["bad_vertex"]), info["n_clusters"]]
    print(f"{tag} h = {h}: V {len(v)} -> {counts[0]}, T {len(t)} -> {counts[1]}, degenerate {counts[2]}, duplicate {counts[3]}, "
          f"flags {counts[4]}, clusters {counts[5]}; reference {want['counts']}")
    assert counts == want["counts"], tag
    assert info["n_vertices"][0] == len(v) and info["n_triangles"][0] == len(t) and info["cell_size"] == h and info["tried"] == []
    assert np.array_equal(_np(info["origin"]), want["origin"]), f"{tag}: origin"
    for k, dt in (("vertices", torch.float64), ("triangles", torch.int32), ("vertex_index", torch.int64),
                  ("vertex_cluster", torch.int32), ("triangle_index", torch.int64)):
        assert got[k].dtype == dt and _np(got[k]).shape == want[k].shape, f"{tag}: {k} {tuple(got[k].shape)} {want[k].shape}"
        assert np.array_equal(_np(got[k]), want[k], equal_nan=(k == "vertices")), f"{tag}: {k}"
    # attributes: a gather with vertex_index
    index = _np(got["vertex_index"])
    assert np.array_equal(_np(got["attributes"]["id"]), index.astype(np.float32))
    assert np.array_equal(_np(got["attributes"]["pair"]), _np(attrs["pair"])[index], equal_nan=True)
    assert np.array_equal(_np(got["vertices"]), v[index], equal_nan=True)
    if twice:
        again = R.simplify_mesh(_dev(v), _dev(t), cell_size=h, **kw)
        for k in ("vertices", "triangles", "vertex_index", "vertex_cluster", "triangle_index"):
            assert np.array_equal(_np(again[k]), _np(got[k]), equal_nan=True), f"{tag}: {k} differs between two runs"
        assert again["info"]["n_clusters"] == info["n_clusters"] and again["info"]["n_duplicate"] == info["n_duplicate"]
    return got, want


# ---- hand-made meshes -----------------------------------------------------------------------------------------------------
def test_a_strip_where_one_triangle_collapses_to_an_edge(R):
    # vertices 1 and 2 share cell (1, 0, 0): the middle triangle keeps two clusters only
    v = [[0.2, 0.2, 0.0], [1.2, 0.3, 0.0], [1.7, 0.8, 0.0], [2.5, 0.5, 0.0], [0.5, 1.5, 0.0]]
    t = [[0, 1, 4], [1, 2, 4], [2, 3, 4]]
    got, want = _check(R, v, t, 1.0, (0.0, 0.0, 0.0), tag="strip")
    assert want["counts"] == [4, 2, 1, 0, 0, 4] and _np(got["triangle_index"]).tolist() == [0, 2]
    assert _np(got["vertex_cluster"]).tolist() == [0, 1, 1, 2, 3]


@pytest.mark.parametrize("order", ["forward", "swapped"])
def test_same_cluster_triple_opposite_orientation_the_smaller_index_survives(R, order):
    v = [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.6, 0.4, 0.5], [1.4, 0.6, 0.5], [0.4, 1.6, 0.5]]
    t = [[0, 1, 2], [5, 4, 3]]                                # the second: the same three cells, the other way round
    if order == "swapped":
        t = t[::-1]
    got, want = _check(R, v, t, 1.0, (0.0, 0.0, 0.0), tag="opposite " + order)
    assert want["counts"][:4] == [3, 1, 0, 1] and _np(got["triangle_index"]).tolist() == [0]
    # corner order kept: the survivor is the input's first triangle through the cluster map
    assert np.array_equal(_np(got["triangles"])[0], _np(got["vertex_cluster"])[np.array(t[0])])


def test_two_members_at_equal_d2_the_smaller_index_wins(R):
    # cell (0,0,0) holds vertices 3 and 1 at mirror positions about their mean; listed so that the larger index comes first
    v = [[1.5, 0.5, 0.5], [0.75, 0.5, 0.5], [0.5, 1.5, 0.5], [0.25, 0.5, 0.5], [1.5, 1.5, 0.5]]
    t = [[3, 0, 2], [1, 4, 2]]
    got, want = _check(R, v, t, 1.0, (0.0, 0.0, 0.0), tag="tie")
    cluster = _np(got["vertex_cluster"])
    assert cluster[1] == cluster[3] and _np(got["vertex_index"])[cluster[1]] == 1
    assert want["counts"][5] == 4 and want["counts"][1] == 2


def test_cell_faces_and_negative_indices_floor_not_truncation(R):
    # x = 1.0 lies on a face (it belongs to cell 1); with the origin at 0.75 the vertices at 0.5 and 0.25 have index -1,
    # the one at 0.8 index 0: truncation would put all three into cell 0
    v = [[1.0, 0.0, 0.0], [0.5, 2.0, 0.0], [0.25, 0.1, 2.0], [0.8, 0.2, 2.1], [3.0, 3.0, 3.0], [-2.0, -2.0, -2.0]]
    t = [[0, 1, 2], [3, 4, 5], [2, 3, 4]]
    for origin in ((0.0, 0.0, 0.0), (0.75, 0.0, 0.0), (0.75, 2.5, 2.5)):
        _check(R, v, t, 1.0, origin, tag=f"faces {origin}")
    i, _, _ = S.cells(np.array(v), (0.75, 0.0, 0.0), 1.0)
    assert i[:4, 0].tolist() == [0, -1, -1, 0]
    got, want = _check(R, v, t, 1.0, (0.75, 0.0, 0.0), tag="faces")
    assert want["counts"][5] == 6 and want["counts"][1] == 3, "2 and 3 are different clusters"


def test_everything_in_one_cell_gives_an_empty_output(R):
    v, t = F.isolated(7, seed=2)
    got, want = _check(R, v * 0.01, t, 100.0, (-50.0, -50.0, -50.0), tag="one cell")
    assert want["counts"] == [0, 0, 7, 0, 0, 1] and got["vertices"].shape == (0, 3) and got["triangles"].shape == (0, 3)
    assert (_np(got["vertex_cluster"]) == -1).all()


def test_no_triangles_and_no_vertices(R):
    d = device()
    for V in (0, 5):
        v = torch.rand(V, 3, dtype=torch.float64, device=d)
        t = torch.zeros(0, 3, dtype=torch.int32, device=d)
        out = R.simplify_mesh(v, t, cell_size=0.5, attributes={"a": torch.zeros(V, 2, device=d)})
        assert out["vertices"].shape == (0, 3) and out["triangles"].shape == (0, 3) and out["vertex_index"].shape == (0,)
        assert out["vertex_cluster"].shape == (V,) and (out["vertex_cluster"] == -1).all()
        assert out["triangle_index"].shape == (0,) and out["attributes"]["a"].shape == (0, 2)
        info = out["info"]
        assert info["n_clusters"] == 0 and info["n_vertices"] == (V, 0) and info["n_triangles"] == (0, 0)
        want = S.simplify(_np(v), _np(t), 0.5)
        assert want["counts"] == [0, 0, 0, 0, 0, 0] and np.array_equal(_np(info["origin"]), want["origin"])
    # triangles without any vertex: every index is out of range
    v0 = torch.zeros(0, 3, dtype=torch.float64, device=d)
    with pytest.raises(ValueError, match="outside"):
        R.simplify_mesh(v0, torch.zeros(3, 3, dtype=torch.int32, device=d), cell_size=1.0)


def test_bad_vertices_and_bad_indices_are_flagged_and_the_neighbours_left_intact(R):
    v0, t0 = F.isolated(6, seed=4)
    h, origin = 0.05, (-10.0, -10.0, -10.0)
    clean = S.simplify(v0, t0, h, origin)
    assert clean["counts"][:5] == [18, 6, 0, 0, 0]
    for bad in (np.nan, np.inf, -np.inf, origin[0] + h * 2.0 ** 20, origin[0] - h * (2.0 ** 20 + 1)):
        v = v0.copy()
        v[4, 0] = bad                                         # triangle 1
        got, want = _check(R, v, t0, h, origin, tag=f"bad vertex {bad}")
        assert want["counts"][:5] == [15, 5, 0, 0, 2] and _np(got["triangle_index"]).tolist() == [0, 2, 3, 4, 5]
        assert _np(got["vertex_cluster"])[3:6].tolist() == [-1, -1, -1]
        keep = np.r_[0:3, 6:18]
        assert np.array_equal(_np(got["vertices"]), v0[keep])
    # the last usable cell index
    v = v0.copy()
    v[4, 0] = origin[0] + h * (2.0 ** 20 - 0.5)
    assert _check(R, v, t0, h, origin, tag="last cell")[1]["counts"][:5] == [18, 6, 0, 0, 0]
    # the default origin ignores the non-finite vertex
    v = v0.copy()
    v[4] = (np.nan, -1e30, 0.0)
    got, want = _check(R, v, t0, h, tag="default origin, NaN row")
    assert np.array_equal(want["origin"], np.delete(v0, 4, axis=0).min(axis=0)) and want["counts"][4] == 2
    # an index outside [0, V): ValueError, as clean_mesh has it, and the next valid call is exact
    for bad in (-1, len(v0), 2 ** 31 - 1):
        t = t0.copy()
        t[2, 1] = bad
        with pytest.raises(ValueError, match="outside"):
            R.simplify_mesh(_dev(v0), _dev(t), cell_size=h)
        assert S.simplify(v0, t, h, origin)["counts"][4] == 1
    _check(R, v0, t0, h, origin, ref=clean, tag="after the bad index")


def test_an_unreferenced_vertex_in_a_populated_cell_does_not_move_the_mean(R):
    # cell (0,0,0): members 0 (0.2) and 3 (0.6), mean 0.4 -> 3 is... both 0.2 away; with the unreferenced 5 (0.9) counted the
    # mean would be 0.567 and 3 the clear winner.  Made asymmetric: 0 at 0.3 wins only when 5 is ignored.
    v = [[0.3, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.6, 0.5, 0.5], [1.5, 1.5, 0.5], [0.95, 0.5, 0.5], [0.1, 0.5, 0.5]]
    t = [[0, 1, 2], [3, 4, 2], [6, 1, 4]]
    got, want = _check(R, v, t, 1.0, (0.0, 0.0, 0.0), tag="unreferenced")
    # members 0.3, 0.6, 0.1: mean 1/3 -> vertex 0; with 0.95 the mean would be 0.4875 -> vertex 3
    assert _np(got["vertex_index"])[0] == 0 and _np(got["vertex_cluster"])[5] == -1


# ---- a hub --------------------------------------------------------------------------------------------------------------
_hub = S.hub


@pytest.mark.parametrize("double", [False, True])
def test_a_hub_of_4096_fan_triangles(R, double):
    v, t = _hub(double)
    got, want = _check(R, v, t, 1.0, (0.0, 0.0, 0.0), tag=f"hub double={double}", twice=True)
    assert want["counts"] == [8193, 4096, 0, 4096 if double else 0, 0, 8193]
    assert _np(got["triangle_index"]).tolist() == list(range(0, len(t), 2 if double else 1))


# ---- the cleanup tests' volumes through the device marching cubes -------------------------------------------------------
def _mc(R, name):
    if name not in _MC:
        u = {"A": F.volume_a, "noise": F.noise_volume,
             "shell128": lambda: -(np.abs(sphere(128, 0.8, (0.0, 0.0, 0.0))) - 0.08).astype(np.float32)}[name]()
        v, t = R.marching_cubes(_dev(u), 0.0)
        _MC[name] = _arrays(_np(v), _np(t))
    return _MC[name]


@pytest.mark.parametrize("h", [1.5, 2.5, 4.0])
@pytest.mark.parametrize("name", ["A", "noise"])
def test_marching_cubes_volumes(R, name, h):
    v, t = _mc(R, name)
    for origin in ((-0.37, 0.21, -1.13), None):
        got, want = _check(R, v, t, h, origin, tag=f"{name} origin {origin}", twice=True)
        nv, nt, n_deg, n_dup, flags, n_clusters = want["counts"]
        assert flags == 0 and 0 < nt < len(t) and nt + n_deg + n_dup == len(t) and nv <= n_clusters


def test_many_workgroups_insert_concurrently(R):
    v, t = _mc(R, "shell128")
    assert len(t) >= 2 ** 17, len(t)
    got, want = _check(R, v, t, 2.0, tag="shell128", twice=True)
    assert 0 < want["counts"][1] < len(t) // 2


def test_a_tiny_cell_is_the_cleanup_with_no_criteria(R):
    for name in ("A", "noise"):
        v, t = _mc(R, name)
        out = R.simplify_mesh(_dev(v), _dev(t), cell_size=2.0 ** -12)
        ref = R.clean_mesh(_dev(v), _dev(t))
        for k in ("vertices", "triangles", "vertex_index"):
            assert torch.equal(out[k], ref[k]), (name, k)
        assert out["info"]["n_degenerate"] == 0 and out["info"]["n_duplicate"] == 0
        assert torch.equal(out["triangle_index"], torch.arange(len(t), device=device()))


@pytest.mark.parametrize("h", [1.5, 4.0])
def test_the_output_lies_within_a_cell_diagonal_of_the_input(R, h):
    v, t = _mc(R, "A")
    out = R.simplify_mesh(_dev(v), _dev(t), cell_size=h)
    index = R.MeshIndex(_dev(v), _dev(t))
    pts = R.sample_surface(out["vertices"], out["triangles"], 20000, seed=7)["points"]
    worst = float(index.closest(pts)["distance"].max())
    bound = math.sqrt(3.0) * h * (1.0 + 2.0 ** -40)
    back = R.sample_surface(_dev(v), _dev(t), 20000, seed=8)["points"]
    other = float(R.MeshIndex(out["vertices"], out["triangles"]).closest(back)["distance"].max())
    print(f"h = {h}: output -> input at most {worst:.4f} (bound {bound:.4f}); input -> output at most {other:.4f} (not bounded)")
    assert worst <= bound


# ---- target_triangles -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 1000, 3703])
def test_target_triangles(R, n):
    v, t = _mc(R, "A")
    out = R.simplify_mesh(_dev(v), _dev(t), target_triangles=n, attributes={"id": _dev(np.arange(len(v)))})
    info = out["info"]
    tried = info["tried"]
    print(f"target {n}: T' = {info['n_triangles'][1]} at r = {info['resolution']}, tried {tried}")
    assert 0 < out["triangles"].shape[0] <= n and info["n_triangles"] == (len(t), out["triangles"].shape[0])
    assert 1 <= len(tried) <= 21 and len({r for r, _ in tried}) == len(tried)
    r = max(r for r, nt in tried if 0 < nt <= n)
    assert r == info["resolution"] and dict(tried)[r] == out["triangles"].shape[0]
    origin, L = S.target_grid(v)
    assert info["cell_size"] == L / r and np.array_equal(_np(info["origin"]), origin)
    for kw in ({}, {"origin": tuple(origin.tolist())}):
        same = R.simplify_mesh(_dev(v), _dev(t), cell_size=L / r, **kw)
        for k in ("vertices", "triangles", "vertex_index", "vertex_cluster", "triangle_index"):
            assert torch.equal(same[k], out[k]), k
    want = S.simplify(v, t, L / r, origin)
    assert np.array_equal(_np(out["triangles"]), want["triangles"]) and np.array_equal(_np(out["vertices"]), want["vertices"])
    assert np.array_equal(_np(out["attributes"]["id"]), want["vertex_index"])


def test_target_triangles_above_the_size_returns_the_input(R):
    v, t = F.with_unreferenced()
    for n in (len(t), len(t) + 5):
        out = R.simplify_mesh(_dev(v), _dev(t), target_triangles=n)
        v1, t1, index, _, _ = F.clean(v, t)
        assert np.array_equal(_np(out["vertices"]), v1) and np.array_equal(_np(out["triangles"]), t1)
        assert np.array_equal(_np(out["vertex_index"]), index) and out["info"]["tried"] == []
        assert np.array_equal(_np(out["triangle_index"]), np.arange(len(t)))
        cluster = np.full(len(v), -1)
        cluster[index] = np.arange(len(index))
        assert np.array_equal(_np(out["vertex_cluster"]), cluster) and out["vertex_cluster"].dtype == torch.int32
    # two congruent triangles half the box apart, coordinates on a lattice of 1/2 with L = 2: at h = 2 / r they survive
    # together (every power of two from 4 up) or collapse together (r = 2, 3): no r the bisection tries gives T' = 1
    v2 = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [1.5, 0, 0], [2.0, 0, 0], [1.5, 0.5, 0]], dtype=np.float64)
    t2 = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)
    origin, L = S.target_grid(v2)
    path = [2 ** k for k in range(19, 1, -1)] + [2, 3]
    assert L == 2.0 and [S.simplify(v2, t2, L / r, origin)["counts"][1] for r in path] == [2] * 18 + [0, 0]
    with pytest.raises(ValueError, match="no resolution"):
        R.simplify_mesh(_dev(v2), _dev(t2), target_triangles=1)


# ---- the renderer -----------------------------------------------------------------------------------------------------------
def _tiny_renderer(R):
    from rnb_neus_fork_amd import checkpoint as CK
    dev = device()
    z = np.load(os.path.join(GOLDEN, "ref_ckpt_tiny_step3.npz"), allow_pickle=False)
    nc = z["nerf.conf"]
    torch.manual_seed(99)
    nerf = R.NeRF(D=int(nc[0]), W=int(nc[1]), d_in=int(nc[2]), d_in_view=int(nc[3]), multires=int(nc[4]),
                  multires_view=int(nc[5]), output_ch=int(nc[6]), skips=[int(nc[7])], use_viewdirs=True).to(dev)
    sdf = R.SDFNetwork(d_in=3, d_out=65, d_hidden=64, n_layers=8, skip_in=[4], multires=6).to(dev)
    devn = R.SingleVarianceNetwork(0.1).to(dev)
    col = R.RenderingNetwork(d_feature=64, mode="no_view_dir", d_in=6, d_out=3, d_hidden=64, n_layers=2, multires_view=4).to(dev)
    ren = R.NeuSRenderer(nerf, sdf, devn, col, n_samples=16, n_importance=16, n_outside=0, up_sample_steps=4, perturb=1.0)
    params = list(nerf.parameters()) + list(sdf.parameters()) + list(devn.parameters()) + list(col.parameters())
    CK.load_checkpoint(os.path.join(GOLDEN, "ref_ckpt_tiny.pth"), nerf, sdf, devn, col, R.FlatAdam(params, lr=1.0), map_location=dev)
    return ren


def test_the_renderer_simplify_keyword(R):
    from tests.mesh_attrs_util import HI, LO
    ren = _tiny_renderer(R)
    res, h = 48, 2.5
    plain_v, plain_t = ren.extract_geometry(LO, HI, res, threshold=0.0, backend="native")
    assert ren.last_mesh_simplify is None and len(plain_t) > 1000
    gv, gt = R.marching_cubes(ren.extract_fields(LO, HI, res, to_host=False), 0.0)
    want = R.simplify_mesh(gv, gt, cell_size=h)
    assert 0 < want["triangles"].shape[0] < len(plain_t) // 2
    index = _np(want["vertex_index"])
    sv, st = ren.extract_geometry(LO, HI, res, threshold=0.0, backend="native", simplify=dict(cell_size=h))
    info = ren.last_mesh_simplify
    assert info["n_triangles"] == (len(plain_t), len(st)) and info["cell_size"] == h
    assert sv.dtype == np.float64 and st.dtype == np.int32
    # simplify_mesh applied to the result without `simplify`: the same vertices picked, the same triangles
    assert np.array_equal(st, _np(want["triangles"])) and np.array_equal(sv, plain_v[index])
    # after the cleaning
    cv, ct = ren.extract_geometry(LO, HI, res, threshold=0.0, backend="native", clean={"keep_largest": 1},
                                  simplify=dict(cell_size=h))
    cleaned = R.clean_mesh(gv, gt, keep_largest=1)
    both = R.simplify_mesh(cleaned["vertices"], cleaned["triangles"], cell_size=h)
    assert np.array_equal(ct, _np(both["triangles"]))
    assert np.array_equal(cv, plain_v[_np(cleaned["vertex_index"])[_np(both["vertex_index"])]])
    # target_triangles through the keyword
    tv, tt = ren.extract_geometry(LO, HI, res, threshold=0.0, backend="native", simplify=dict(target_triangles=500))
    assert 0 < len(tt) <= 500 and len(ren.last_mesh_simplify["tried"]) <= 21
    # the textured path: the attributes are those of the surviving vertices alone, bit for bit
    tex = ren.extract_textured_geometry(LO, HI, res, simplify=dict(cell_size=h))
    assert np.array_equal(tex["triangles"], st) and np.array_equal(tex["vertices"], sv)
    direct = ren.vertex_attributes(grid_vertices=want["vertices"], bounds=(LO, HI), resolution=res)
    for k_tex, k_at in (("normals", "normal"), ("sdf", "sdf"), ("albedo", "albedo"), ("colors", "rgb")):
        assert np.array_equal(tex[k_tex], _np(direct[k_at])), k_tex
    assert len(tex["normals"]) == len(sv)
    # simplify=None: both calls behave as before
    plain = ren.extract_textured_geometry(LO, HI, res)
    assert np.array_equal(plain["triangles"], plain_t) and np.array_equal(plain["vertices"], plain_v)
