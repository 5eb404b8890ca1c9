"""Mesh ray casting on the device (csrc/mesh_raycast.hip through `MeshIndex.raycast`, `.interpolate`, `.visible`,
`mesh_view_maps`, `normal_angular_error`) against the brute-force numpy reference of tests/mesh_raycast_ref.py.

Kernel and reference evaluate the same watertight pair test, both in IEEE fp64 without contraction, and the result of a
ray is the minimum under (t, index) over all triangles: `t`, `triangle` and `bary` are required BIT-EQUAL to the
reference, and bit-equal between any two grids of the same mesh — only a walk that skipped a cell can differ, which needs
no reference to see.  References are computed once and shared; callers must not modify what they get."""
import math

import numpy as np
import pytest
import torch

from tests import mesh_raycast_ref as F
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device

pytestmark = pytest.mark.gpu

KEYS = ("t", "triangle", "bary")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device())


def _index(R, v, t, cells=None, grid=None):
    return R.MeshIndex(_dev(np.asarray(v, dtype=np.float64).reshape(-1, 3)), _dev(np.asarray(t, dtype=np.int32).reshape(-1, 3)),
                       cells=cells, grid=grid)


def _cast(index, o, d, lo=None, hi=None):
    """(t, triangle, bary) as numpy, after checking what the other outputs owe them"""
    o, d = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    out = index.raycast(_dev(o), _dev(d), None if lo is None else _dev(lo), None if hi is None else _dev(hi))
    assert out["t"].dtype == torch.float64 and out["triangle"].dtype == torch.int32 and out["bary"].dtype == torch.float64
    assert out["hit"].dtype == torch.bool and out["point"].shape == (len(o), 3) and out["normal"].shape == (len(o), 3)
    t, tri, bary = (out[k].cpu().numpy() for k in KEYS)
    hit = tri >= 0
    assert np.array_equal(out["hit"].cpu().numpy(), hit)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(out["point"].cpu().numpy(), np.where(hit[:, None], o + t[:, None] * d, np.nan), equal_nan=True)
    assert np.isnan(out["normal"].cpu().numpy()[~hit]).all() and np.isnan(bary[~hit]).all()
    return t, tri, bary


def _same(a, b, what):
    for x, y, k in zip(a, b, KEYS):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), \
            f"{what}: {k} differs in {int((~((x == y) | ((x != x) & (y != y)))).sum())} places"


def _torus_index(R, cells=None, grid=None):
    case = F.torus_rays()
    return _index(R, case["vertices"], case["triangles"], cells=cells, grid=grid)


def test_parity_with_the_brute_force_reference(R):
    case = F.torus_rays()
    v, t = case["vertices"], case["triangles"]
    assert t.shape == (1200, 3) and len(case["origins"]) == 2000
    index = _torus_index(R)
    assert index.n_cells > 100 and index.covers and not index.skipped
    got = _cast(index, case["origins"], case["directions"], case["t_min"], case["t_max"])
    ref = case["ref"]
    hit = ref[1] >= 0
    print(f"torus: {int(hit.sum())} of {len(hit)} rays hit; t differs from the reference in {int((got[0] != ref[0]).sum())} places, "
          f"triangle in {int((got[1] != ref[1]).sum())}, bary in {int((got[2] != ref[2])[hit].sum())}")
    _same(got, ref, "torus against the reference")
    # the face normal is the hit triangle's, and float32 rays are the same rays widened
    nrm = index.raycast(_dev(case["origins"]), _dev(case["directions"]), _dev(case["t_min"]), _dev(case["t_max"]))["normal"].cpu().numpy()
    assert np.abs(nrm[hit] - F.face_normals(v, t)[ref[1][hit]]).max() <= 8 * F.EPS
    o32, d32 = case["origins"].astype(np.float32), case["directions"].astype(np.float32)
    out32 = index.raycast(_dev(o32), _dev(d32))
    _same(tuple(out32[k].cpu().numpy() for k in KEYS), F.raycast_all(o32.astype(np.float64), d32.astype(np.float64), v, t), "float32 rays")
    # scalar bounds are the same bounds
    o, d = case["origins"][500:1000], case["directions"][500:1000]
    out = index.raycast(_dev(o), _dev(d), 0.25, 0.9)
    _same(tuple(out[k].cpu().numpy() for k in KEYS), F.raycast_all(o, d, v, t, 0.25, 0.9), "scalar bounds")
    # so are one-element tensors, a single ray included, and [N,1] columns (the near / far of view_rays)
    for n in (1, 7):
        want = F.raycast_all(o[:n], d[:n], v, t, 0.25, 0.875)               # exact in float32 too
        for lo, hi in ((torch.tensor(0.25), torch.tensor([0.875])), (torch.full((n, 1), 0.25), torch.full((n,), 0.875, dtype=torch.float64))):
            out = index.raycast(_dev(o[:n]), _dev(d[:n]), lo.to(device()), hi.to(device()))
            _same(tuple(out[k].cpu().numpy() for k in KEYS), want, f"tensor bounds, {n} rays")


def test_results_do_not_depend_on_the_grid(R):
    case = F.torus_rays()
    v, t = case["vertices"], case["triangles"]
    args = (case["origins"], case["directions"], case["t_min"], case["t_max"])
    brute = _torus_index(R, cells=1)
    assert brute.dims == (1, 1, 1) and brute.n_entries == 1200
    base = _cast(brute, *args)
    _same(base, case["ref"], "cells=1 against the reference")
    for cells in (2, (7, 3, 5), None):
        index = _torus_index(R, cells=cells)
        assert index.covers
        _same(_cast(index, *args), base, f"cells={cells} against brute force (cells=1)")
    _same(_cast(_torus_index(R), *args), base, "a second run of the default grid")
    # a grid placed by hand that still covers the mesh (off the mesh's box, cells that do not divide it)
    lo, hi = v.min(axis=0), v.max(axis=0)
    hand = _torus_index(R, grid=(lo - 0.173, 0.131, tuple(int(x) for x in np.ceil((hi - lo + 0.4) / 0.131))))
    assert hand.covers
    _same(_cast(hand, *args), base, "a hand-placed grid that covers the mesh")
    # one over a part of the mesh is refused: its boundary cells hold triangles the walk would not find
    part = _torus_index(R, grid=(lo + 0.5 * (hi - lo), float((hi - lo).max()) / 16, (3, 2, 4)))
    assert not part.covers
    with pytest.raises(ValueError, match="without grid="):
        part.raycast(_dev(args[0]), _dev(args[1]))


def test_rays_on_cell_faces_and_through_cell_corners(R):
    """rays lying exactly in the planes between cells of the default grid, along cell edges and through cell corners,
    axis-parallel (zeros in d) and diagonal, starting inside the box, outside it, and pointing away from it"""
    case = F.torus_rays()
    index, brute = _torus_index(R), _torus_index(R, cells=1)
    o0, c, dims = np.array(index.origin), index.cell_size, index.dims
    assert min(dims) >= 3
    planes = [o0[k] + np.arange(dims[k] + 1) * c for k in range(3)]
    mids = [o0[k] + (np.arange(dims[k]) + 0.5) * c for k in range(3)]
    os_, ds_ = [], []
    for m in range(3):
        u, w = (m + 1) % 3, (m + 2) % 3
        for cu, cw in ((planes[u], planes[w]), (planes[u], mids[w]), (mids[u], planes[w])):       # edges; the two kinds of faces
            gu, gw = (x.reshape(-1) for x in np.meshgrid(cu, cw, indexing="ij"))
            for start, sign in ((planes[m][0] - 1.5 * c, 1.0), (planes[m][-1] + 0.7 * c, -1.0), (planes[m][dims[m] // 2], 1.0),
                                (planes[m][dims[m] // 2], -1.0), (planes[m][-1] + 0.7 * c, 1.0)):      # the last points away
                o = np.zeros((len(gu), 3))
                o[:, u], o[:, w], o[:, m] = gu, gw, start
                d = np.zeros((len(gu), 3))
                d[:, m] = sign * 0.75
                os_.append(o)
                ds_.append(d)
    # diagonals through every cell corner, starting on it, before the box and behind it
    lattice = np.stack(np.meshgrid(*planes, indexing="ij"), axis=-1).reshape(-1, 3)
    for dirn in ((1, 1, 1), (1, -1, 1), (-1, 1, 0), (0, 1, -1), (1, 0, 1), (-1, -1, -1)):
        dirn = np.array(dirn, dtype=np.float64) * c
        for shift in (0.0, -float(max(dims)), 3.0):
            os_.append(lattice + shift * dirn)
            ds_.append(np.tile(dirn, (len(lattice), 1)))
    o, d = np.concatenate(os_), np.concatenate(ds_)
    lo = np.full(len(o), -np.inf)
    lo[::2] = 0.0                                              # half of them lines
    got, base = _cast(index, o, d, lo), _cast(brute, o, d, lo)
    n_hit = int((base[1] >= 0).sum())
    print(f"cell faces: {len(o)} rays, {n_hit} hit")
    assert n_hit > len(o) // 20 and (base[1] < 0).sum() > len(o) // 20
    _same(got, base, "rays on cell faces against brute force (cells=1)")
    sub = np.arange(0, len(o), 23)
    _same(tuple(x[sub] for x in base), F.raycast_all(o[sub], d[sub], case["vertices"], case["triangles"], lo[sub]), "cell faces, reference")
    # the anisotropic torus: cubic cells one wide on one axis, hundreds on another
    s = np.array([1.0, 0.01, 30.0])
    vs = case["vertices"] * s
    args = (case["origins"] * s, case["directions"] * s, case["t_min"], case["t_max"])
    base = _cast(_index(R, vs, case["triangles"], cells=1), *args)
    for cells in ((7, 3, 5), None):
        _same(_cast(_index(R, vs, case["triangles"], cells=cells), *args), base, f"scaled torus, cells={cells}")


def test_a_closed_surface_has_no_pinholes(R):
    case = F.watertight_case()
    v, t = case["vertices"], case["triangles"]
    index = _index(R, v, t)
    assert index.n_cells > 1
    got = _cast(index, case["origins"], case["directions"])
    assert len(got[0]) == 3 * 2562
    assert (got[1] >= 0).all(), f"{int((got[1] < 0).sum())} rays through vertices and edges of a closed surface miss it"
    _same(got, case["ref"], "icosphere against the reference")
    _same(_cast(_index(R, v, t, cells=1), case["origins"], case["directions"]), case["ref"], "icosphere, cells=1")


def test_degenerate_triangles_and_non_finite_input(R):
    rng = np.random.default_rng(9)
    a, b, c = np.array([0.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.25]), np.array([0.0, 1.0, -0.25])
    # One real triangle among zero-area ones.  Two or three equal corners: the sheared corners are equal too, one edge
    # function is exactly 0 and the other two exactly opposite, det == 0, never hit.  Collinear, distinct corners have
    # det == 0 in exact arithmetic only: a ray through their segment itself, to within rounding, sees three edge
    # functions that are rounding noise, and may be given a hit with a t somewhere inside the triangle's extent along
    # the ray (include/rnbneus.h says so).  Rays that pass such a triangle by never hit it, on any grid; for the rays
    # aimed at the segment the pair test alone is checked, through the one-cell grid, against the reference.
    v = np.array([a, b, c, 0.5 * (a + b), 0.25 * (a + c), b + 0.5 * (c - b)])
    t_equal = np.array([[0, 0, 1], [1, 2, 2], [2, 2, 2], [0, 1, 2], [1, 0, 1]], dtype=np.int32)
    t = np.array([[0, 0, 1], [0, 3, 1], [2, 2, 2], [0, 1, 2], [1, 5, 2], [0, 4, 2]], dtype=np.int32)
    tgt = np.concatenate([rng.uniform(-0.2, 1.2, (300, 3)) * [1, 1, 0], v, 0.5 * (v[t[:, 0]] + v[t[:, 1]]),
                          a + rng.uniform(0, 1, (200, 1)) * (b - a)])
    o = rng.normal(size=(len(tgt), 3)) + [0, 0, 3.0]
    d = tgt - o
    ref = F.raycast_all(o, d, v, t_equal)
    assert set(np.unique(ref[1])) == {-1, 3}, "a triangle with equal corners is never hit"
    for cells in (None, 1, 3):
        _same(_cast(_index(R, v, t_equal, cells=cells), o, d), ref, f"equal corners, cells={cells}")
    flat = F.raycast_all(o, d, v, t)
    assert set(np.unique(flat[1][:300])) == {-1, 3}, "a ray that passes a collinear triangle by does not hit it"
    for cells in (None, 1, 3):
        _same(_cast(_index(R, v, t, cells=cells), o[:300], d[:300]), tuple(x[:300] for x in flat), f"collinear corners, cells={cells}")
    _same(_cast(_index(R, v, t, cells=1), o, d), flat, "collinear corners, rays aimed at the segments, the pair test alone")
    # a triangle with a non-finite vertex is skipped
    t = t_equal
    v2 = np.concatenate([v, [[np.inf, 0.0, 0.0], [0.5, 0.5, np.nan]]])
    t2 = np.concatenate([t, [[0, 1, 6], [7, 1, 2]]]).astype(np.int32)
    index = _index(R, v2, t2)
    assert index.skipped and index.covers
    _same(_cast(index, o, d), ref, "a skipped triangle")
    # rays that are not rays
    bad_o, bad_d = np.tile(o[:8], (1, 1)), np.tile(d[:8], (1, 1))
    bad_o[0, 1], bad_o[1, 2], bad_d[2, 0], bad_d[3, 1], bad_d[4] = np.nan, np.inf, np.nan, -np.inf, 0.0
    lo, hi = np.zeros(8), np.full(8, np.inf)
    lo[5], hi[6] = np.nan, np.nan
    got = _cast(index, bad_o, bad_d, lo, hi)
    assert np.isnan(got[0][:7]).all() and (got[1][:7] == -1).all() and np.isnan(got[2][:7]).all()
    _same(got, F.raycast_all(bad_o, bad_d, v, t, lo, hi), "non-finite rays")
    assert got[0][7] == ref[0][7]
    # t_min > t_max, t_max = -inf, t_min = +inf: nothing in range
    for lo1, hi1 in ((2.0, 1.0), (0.0, -np.inf), (np.inf, np.inf)):
        got = _cast(index, o[:64], d[:64], np.full(64, lo1), np.full(64, hi1))
        assert np.isposinf(got[0]).all() and (got[1] == -1).all()
    # no ray
    out = index.raycast(_dev(np.zeros((0, 3))), _dev(np.zeros((0, 3))))
    assert all(out[k].shape[0] == 0 for k in ("t", "triangle", "bary", "hit", "point", "normal"))
    # no triangle, and none that is usable: every ray misses
    for ve, te in ((np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32)), (v2[6:], np.array([[0, 1, 1]], dtype=np.int32))):
        empty = _index(R, ve, te)
        assert empty.n_entries == 0
        got = _cast(empty, bad_o, bad_d, lo, hi)
        assert np.isnan(got[0][:7]).all() and np.isposinf(got[0][7]) and (got[1] == -1).all() and np.isnan(got[2]).all()


def _facet_angle(v, t):
    """the largest angle at the centre between two corners of one triangle of a mesh inscribed in the unit sphere"""
    e = F.mesh_edges(t)
    return float(np.arccos(np.clip((v[e[:, 0]] * v[e[:, 1]]).sum(axis=1), -1.0, 1.0)).max())


def test_view_maps_of_an_icosphere(R):
    v, t = F.icosphere(2)
    index = _index(R, v, t)
    H, W = 12, 16
    o, d = F.pinhole_rays(H, W, eye=(2.4, -1.1, 0.9), look_at=(0.1, 0.0, 0.05), fov_deg=50.0)
    ref_t, ref_tr, ref_b = F.raycast_all(o, d, v, t)
    hit = ref_tr >= 0
    assert 20 < hit.sum() < H * W - 20, "the view holds the silhouette"
    albedo = np.random.default_rng(2).uniform(0.0, 1.0, (len(v), 3))
    maps = R.mesh_view_maps(index, _dev(o), _dev(d), shape=(H, W), vertex_normals=_dev(v), vertex_albedo=_dev(albedo))
    assert maps["mask"].shape == (H, W) and maps["depth"].shape == (H, W) and maps["normal"].shape == (H, W, 3)
    assert maps["face_normal"].shape == (H, W, 3) and maps["albedo"].shape == (H, W, 3)
    got = {k: x.cpu().numpy().reshape((H * W,) + tuple(x.shape[2:])) for k, x in maps.items()}
    assert np.array_equal(got["mask"], hit), "the mask is the reference's hit set"
    assert np.array_equal(got["triangle"], ref_tr)
    length = np.sqrt((d * d).sum(axis=1))
    assert np.isposinf(got["depth"][~hit]).all() and np.abs(got["depth"][hit] - (ref_t * length)[hit]).max() <= 4 * F.EPS * 4.0
    assert np.isnan(got["normal"][~hit]).all() and np.isnan(got["albedo"][~hit]).all() and np.isnan(got["face_normal"][~hit]).all()
    # The vertex normals are the unit positions.  An interpolated normal is a combination with weights >= 0 of the
    # three corner directions; from the centre the hit point P is seen inside the spherical triangle of those corners,
    # whose diameter is its longest side, so each corner direction is within theta_e (the largest edge angle of the
    # mesh) of P's direction, and so is any combination of them with weights >= 0: a cone about P / |P| is convex.
    theta_e = _facet_angle(v, t)
    assert 0.2 < theta_e < 0.4, "the twice-subdivided icosphere: 20.1 degrees at most between neighbours"
    p = (o + ref_t[:, None] * d)[hit]
    p_hat = p / np.linalg.norm(p, axis=1, keepdims=True)
    n = got["normal"][hit]
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 4 * F.EPS
    ang = np.arccos(np.clip((n * p_hat).sum(axis=1), -1.0, 1.0))
    print(f"view maps: {int(hit.sum())} pixels on the mesh; interpolated normal within {np.degrees(ang.max()):.2e} degrees of the hit "
          f"point's direction (facet bound {np.degrees(theta_e):.2f}); face normal within "
          f"{np.degrees(np.arccos((got['face_normal'][hit] * p_hat).sum(axis=1).min())):.2f}")
    assert (ang <= theta_e).all()
    # more than the bound asks: sum of bary_k x corner_k IS the hit point, so with normals = positions the interpolated
    # normal is P / |P| up to rounding (1e-9 rad: arccos near 1 keeps half the digits) — a bary in the wrong order fails here
    assert ang.max() <= 1e-7
    assert np.arccos((got["face_normal"][hit] * p_hat).sum(axis=1).min()) <= theta_e, "a face normal is inside its facet's cone"
    want = (albedo[t[ref_tr[hit]]] * ref_b[hit][:, :, None]).sum(axis=1)
    assert np.abs(got["albedo"][hit] - want).max() <= 8 * F.EPS
    # the dict of `DeviceRays.view_rays` in place of the rays: float32 [n,3] with the grid's H and W
    o32, d32 = o.astype(np.float32), d.astype(np.float32)
    from_dict = R.mesh_view_maps(index, {"rays_o": _dev(o32), "rays_d": _dev(d32), "H": H, "W": W, "near": None}, vertex_normals=_dev(v))
    assert from_dict["mask"].shape == (H, W) and from_dict["normal"].shape == (H, W, 3) and "albedo" not in from_dict
    t32 = F.raycast_all(o32.astype(np.float64), d32.astype(np.float64), v, t)[1]
    assert np.array_equal(from_dict["triangle"].cpu().numpy().reshape(-1), t32)
    # interpolate, flat values
    hits = index.raycast(_dev(o), _dev(d))
    flat = index.interpolate(hits, _dev(albedo[:, 0].copy())).cpu().numpy()
    assert flat.shape == (H * W,) and np.abs(flat[hit] - want[:, 0]).max() <= 8 * F.EPS and np.isnan(flat[~hit]).all()
    # the angular error of a map against itself, and against the same map rotated by a known angle about the view axis
    same = R.normal_angular_error(maps["normal"], maps["normal"], maps["mask"])
    assert same == {"mean": 0.0, "median": 0.0, "rms": 0.0, "count": int(hit.sum())}
    ang0 = math.radians(11.0)
    nn = got["normal"]
    with np.errstate(invalid="ignore"):
        k = np.cross(nn, [0.3, -0.5, 0.81])                                                    # an axis per pixel, perpendicular
        k /= np.linalg.norm(k, axis=1, keepdims=True)                                          # to its normal
        rot = nn * math.cos(ang0) + np.cross(k, nn) * math.sin(ang0)
    e = R.normal_angular_error(maps["normal"], _dev(rot).reshape(H, W, 3), maps["mask"])
    assert e["count"] == int(hit.sum()) and all(abs(e[q] - 11.0) < 1e-9 for q in ("mean", "median", "rms"))
    # the mask of the view decides, not the NaNs alone: half the mask, half the count or less
    half = maps["mask"].clone()
    half[H // 2:] = False
    assert R.normal_angular_error(maps["normal"], _dev(rot).reshape(H, W, 3), half)["count"] == int(hit.reshape(H, W)[:H // 2].sum())


def test_visibility_of_icosphere_vertices_from_outside(R):
    v, t = F.icosphere(2)
    index = _index(R, v, t)
    eye = np.array([1.7, -2.1, 1.3])
    dist = float(np.linalg.norm(eye))
    # On the unit sphere a point is seen from the eye when its angle to the eye's direction is below the horizon's,
    # acos(1 / |eye|).  The mesh is inscribed in the sphere and its facets span at most theta_e at the centre: a facet
    # can hide or bare only what lies within theta_e of the sphere's horizon.  Vertices nearer to it than that are not asserted.
    theta_e = _facet_angle(v, t)
    horizon = math.acos(1.0 / dist)
    angle = np.arccos(np.clip(v @ (eye / dist), -1.0, 1.0))
    front, back = angle < horizon - theta_e, angle > horizon + theta_e
    assert front.sum() > 20 and back.sum() > 60
    vis = index.visible(_dev(v), _dev(eye)).cpu().numpy()
    assert vis.dtype == np.bool_ and vis.shape == (len(v),)
    assert vis[front].all(), f"{int((~vis[front]).sum())} vertices facing the eye are reported hidden"
    assert not vis[back].any(), f"{int(vis[back].sum())} vertices on the far side are reported visible"
    # an eye per point, float32 input, and points that are no points
    eyes = np.tile(eye, (len(v), 1))
    assert np.array_equal(index.visible(_dev(v), _dev(eyes)).cpu().numpy(), vis)
    pts = v.copy()
    pts[0, 0], pts[1] = np.nan, eye
    bad = index.visible(_dev(pts), _dev(eye)).cpu().numpy()
    assert not bad[0] and not bad[1] and np.array_equal(bad[2:], vis[2:])
    # with rel_tol = 0 the point's own triangles hide a share of the front vertices: the tolerance is what it is for
    strict = index.visible(_dev(v), _dev(eye), rel_tol=0.0).cpu().numpy()
    assert not strict[back].any() and (strict <= vis).all()
