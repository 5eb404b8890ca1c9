"""Mesh evaluation on the device (csrc/mesh_eval.hip through `MeshIndex`, `sample_surface`, `mesh_distance`) against the
brute-force numpy reference of tests/mesh_distance_ref.py.

The tolerance rule is that module's: SQUARED distances within 16 x 2^-52 x L^2, L = max |query coordinate| + max |vertex
coordinate|; triangle indices are never compared with the reference's (ties at edges and vertices) — the returned closest
point must lie on the returned triangle and be dist2 away.  Between two runs and between two grids of the SAME mesh
everything is compared bit for bit, indices included: each pair's value is a pure function of its points and the result is
the minimum under (dist2, index), so only a search that stopped too early can differ — which needs no reference to see.
References are computed once and shared; callers must not modify what they get."""
import numpy as np
import pytest
import torch

from tests import mc_shapes
from tests import mesh_distance_ref as F
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device

pytestmark = pytest.mark.gpu

GRIDS = (1, 2, (7, 3, 5), None)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device())


def _np(out):
    return tuple(out[k].cpu().numpy() for k in ("dist2", "closest", "triangle"))


def _query(R, v, t, q, cells=None, grid=None):
    index = R.MeshIndex(_dev(v), _dev(np.asarray(t, dtype=np.int32).reshape(-1, 3)), cells=cells, grid=grid)
    out = index.closest(_dev(q))
    assert out["dist2"].dtype == torch.float64 and out["closest"].dtype == torch.float64 and out["triangle"].dtype == torch.int32
    got = _np(out)
    assert np.array_equal(out["distance"].cpu().numpy(), np.sqrt(got[0]), equal_nan=True)
    return index, got


def _same(a, b, what):
    for x, y, k in zip(a, b, ("dist2", "closest", "triangle")):
        assert np.array_equal(x, y, equal_nan=True), f"{what}: {k} differs in {int((x != y).sum())} places"


def _all_grids_agree(R, v, t, q, what):
    """the same queries under every grid of GRIDS and a second run of the default: bit-equal; returns the default's"""
    index, base = _query(R, v, t, q, cells=1)
    assert index.dims == (1, 1, 1) and index.n_entries == int(F.usable(v, t).sum())
    for cells in GRIDS[1:]:
        index, got = _query(R, v, t, q, cells=cells)
        _same(got, base, f"{what}: cells={cells} against brute force (cells=1)")
        assert index.covers, "a grid built from the mesh's box holds the mesh"
    _same(_query(R, v, t, q)[1], base, f"{what}: two runs")
    # a grid placed by hand over a corner of the mesh's box: what lies outside goes to its boundary cells
    fin = v[np.isfinite(v).all(axis=1)]
    lo, ext = fin.min(axis=0), np.maximum(fin.max(axis=0) - fin.min(axis=0), 1e-3)
    part, got = _query(R, v, t, q, grid=(lo + 0.5 * ext, float(ext.max()) / 16, (3, 2, 4)))
    _same(got, base, f"{what}: a grid over a part of the mesh")
    if len(np.unique(fin, axis=0)) > 1:
        assert not part.covers
    return index, base


def test_parity_with_the_brute_force_reference(R):
    case = F.torus_case()
    v, t, q = case["vertices"], case["triangles"], case["queries"]
    assert t.shape == (1200, 3)
    index, got = _query(R, v, t, q)
    assert index.n_cells > 100 and index.n_entries <= 16 * len(t) + index.n_cells and not index.skipped
    F.check_closest("torus", q, v, t, got, case["ref"][0], F.bound(q, v))
    # one query 50 box sizes away, under its own L
    far = case["far"]
    F.check_closest("torus, far query", far, v, t, _query(R, v, t, far)[1], case["ref_far"][0], F.bound(far, v))
    # queries exactly on cell faces: every corner of every cell of the default grid
    o, c, d = np.array(index.origin), index.cell_size, index.dims
    lattice = np.stack(np.meshgrid(*(o[k] + np.arange(d[k] + 1) * c for k in range(3)), indexing="ij"), axis=-1).reshape(-1, 3)
    ref = F.closest_all(lattice, v, t)
    F.check_closest("torus, cell corners", lattice, v, t, _np(index.closest(_dev(lattice))), ref[0], F.bound(lattice, v))


def test_results_do_not_depend_on_the_grid(R):
    case = F.torus_case()
    v, t = case["vertices"], case["triangles"]
    q = np.concatenate([case["queries"], case["far"], -case["far"], [[0.0, 0.0, 0.0]]])
    index, base = _all_grids_agree(R, v, t, q, "torus")
    assert index.dims != (1, 1, 1)
    # the reference again, through the brute-force grid: what all the grids equal is the right answer
    n = len(case["queries"])
    F.check_closest("torus, every grid", q[:n], v, t, tuple(x[:n] for x in base), case["ref"][0], F.bound(q[:n], v))


def test_shapes_that_stress_the_bins(R):
    case = F.torus_case()
    v, t, q = case["vertices"], case["triangles"], case["queries"]
    # anisotropic: the torus scaled by (1, 0.01, 30): cubic cells are 1 wide in one axis and hundreds in another
    s = np.array([1.0, 0.01, 30.0])
    vs, qs = v * s, q * s
    _, got = _all_grids_agree(R, vs, t, qs, "scaled torus")
    sub = np.arange(0, len(qs), 9)
    F.check_closest("scaled torus", qs[sub], vs, t, tuple(x[sub] for x in got), F.closest_all(qs[sub], vs, t)[0], F.bound(qs, vs))
    # one triangle over the whole box with the 1,200 small ones; then 200 of them: the coarsening rule has to act
    box = np.array([[-2.0, -2.0, -0.5], [2.0, -2.0, 0.5], [0.0, 2.0, 0.0]])
    for n_big, min_rounds in ((1, 1), (200, 2)):
        vb = np.concatenate([v, np.tile(box, (n_big, 1)) + np.repeat(np.arange(n_big), 3)[:, None] * 1e-3])
        tb = np.concatenate([t, len(v) + np.arange(3 * n_big, dtype=np.int32).reshape(-1, 3)])
        index, got = _query(R, vb, tb, q)
        print(f"{n_big} box-wide triangles: dims {index.dims}, E = {index.n_entries}, {index.rounds} counting rounds")
        assert index.n_entries <= 16 * len(tb) + index.n_cells and index.rounds >= min_rounds
        _same(got, _query(R, vb, tb, q, cells=1)[1], f"{n_big} box-wide triangles")
        if n_big == 1:
            F.check_closest("one box-wide triangle", q[sub], vb, tb, tuple(x[sub] for x in got), F.closest_all(q[sub], vb, tb)[0],
                            F.bound(q, vb))
    # T = 1
    v1, t1 = np.array([[0.1, 0.2, 0.3], [0.9, -0.4, 0.5], [-0.3, 0.8, -0.6]]), np.array([[0, 1, 2]], dtype=np.int32)
    _, got = _all_grids_agree(R, v1, t1, q[:600], "one triangle")
    assert (got[2] == 0).all()
    F.check_closest("one triangle", q[:600], v1, t1, got, F.closest_all(q[:600], v1, t1)[0], F.bound(q[:600], v1))
    # every triangle twice: the same distances, and the smaller index of each pair
    _, twice = _query(R, v, np.concatenate([t, t]), q)
    _, once = _query(R, v, t, q)
    _same(twice, once, "duplicated triangles")


def _bin_entries(v, t, origin, cell, dims):
    """The cell rule of the bins in numpy (every triangle usable): the entries as (flat cell, triangle), sorted by both.
    A triangle enters the cells clamp(floor((x - origin) / cell), 0, dim - 1) of its box's two corners and all between."""
    corners, o, d = v[t], np.asarray(origin, dtype=np.float64), np.asarray(dims, dtype=np.int64)
    lo = np.clip(np.floor((corners.min(axis=1) - o) / cell), 0, d - 1).astype(np.int64)
    hi = np.clip(np.floor((corners.max(axis=1) - o) / cell), 0, d - 1).astype(np.int64)
    cells, tris = [], []
    for k in range(len(t)):
        x, y, z = (np.arange(lo[k, a], hi[k, a] + 1) for a in range(3))
        flat = ((z[:, None, None] * d[1] + y[None, :, None]) * d[0] + x[None, None, :]).ravel()
        cells.append(flat)
        tris.append(np.full(len(flat), k, dtype=np.int64))
    cells, tris = np.concatenate(cells), np.concatenate(tris)
    order = np.lexsort((tris, cells))
    return cells[order], tris[order]


def test_bins_past_the_first_chunk_of_the_block_sum_scan(R):
    """More than 2^20 cells: the 64-bit scan of the per-cell counts has 1,041 tiles of 1,024, so the one workgroup that scans
    the tile sums goes through a second chunk of 1,024 and its carry decides where every cell past 2^20 starts.  The torus
    with its flat axis along x (the fastest cell index) under cells = (65, 128, 128): 1,064,960 cells, 371,408 entries,
    3,950 of them in 1,942 non-empty cells at flat indices >= 2^20.  cell_start and the entries are compared as exact
    integers with the cell rule in numpy (the order inside a cell comes from atomics: compared as sets), the queries bit
    for bit with brute force."""
    case = F.torus_case()
    axes = [2, 0, 1]
    v, t = np.ascontiguousarray(case["vertices"][:, axes]), case["triangles"]
    q = np.ascontiguousarray(case["queries"][:, axes])
    dims = (65, 128, 128)
    n_cells = dims[0] * dims[1] * dims[2]
    index, got = _query(R, v, t, q, cells=dims)
    assert index.dims == dims and index.n_cells == n_cells == 1064960 and index.rounds == 1 and not index.skipped and index.covers
    assert (n_cells + 1 + 1023) // 1024 == 1041, "the scan of n_cells + 1 counts has more than 1,024 tiles"
    cells, tris = _bin_entries(v, t, index.origin, index.cell_size, dims)
    counts = np.bincount(cells, minlength=n_cells)
    past = cells >= 2 ** 20
    print(f"{n_cells} cells, E = {len(cells)}; {int(past.sum())} entries in {len(np.unique(cells[past]))} cells past 2^20")
    assert len(cells) == 371408 and int(past.sum()) == 3950 and len(np.unique(cells[past])) == 1942, "the fixture moved"
    assert index.n_entries == len(cells)
    start = index.cell_start.cpu().numpy()
    assert start.dtype == np.int64 and np.array_equal(start, np.concatenate([[0], np.cumsum(counts)])), \
        "cell_start is not the exclusive running sum of the per-cell counts"
    entries = index.entries.cpu().numpy().astype(np.int64)
    got_cells = np.repeat(np.arange(n_cells), np.diff(start))
    order = np.lexsort((entries, got_cells))
    assert np.array_equal(got_cells[order], cells) and np.array_equal(entries[order], tris), "a cell holds other triangles than numpy's"
    _same(got, _query(R, v, t, q, cells=1)[1], "cells=(65, 128, 128) against brute force (cells=1)")


def _segment_d2(p, a, b):
    ab = b - a
    s = np.clip(((p - a) @ ab) / (ab @ ab), 0.0, 1.0)
    r = p - (a + s[:, None] * ab)
    return (r * r).sum(axis=1)


def test_degenerate_triangles_and_non_finite_input(R):
    rng = np.random.default_rng(5)
    q = rng.uniform(-2.0, 2.0, (257, 3))
    a, b = np.array([0.25, -0.5, 0.125]), np.array([1.0, 0.75, -0.5])
    # two equal corners, collinear corners, three equal corners: the distance to the segment / the point
    for name, corners, (s0, s1) in (("two equal corners", [a, a, b], (a, b)), ("collinear", [a, a + 0.25 * (b - a), b], (a, b)),
                                    ("collinear, middle corner last", [a, b, a + 0.5 * (b - a)], (a, b)),
                                    ("a point", [a, a, a], (a, a + 1.0))):
        v, t = np.array(corners), np.array([[0, 1, 2]], dtype=np.int32)
        _, got = _all_grids_agree(R, v, t, q, name)
        want = _segment_d2(q, s0, s1) if name != "a point" else ((q - a) ** 2).sum(axis=1)
        tol = F.bound(q, v)
        assert np.abs(got[0] - want).max() <= tol, name
        F.check_closest(name, q, v, t, got, F.closest_all(q, v, t)[0], tol)
    case = F.torus_case()
    v, t = case["vertices"], case["triangles"]
    q = case["queries"][:257].copy()
    _, clean = _query(R, v, t, q)
    # a NaN / inf query: NaN, NaN, -1, and the neighbouring lanes are intact
    qn = q.copy()
    qn[3, 1], qn[64, 0], qn[200, 2] = np.nan, np.inf, -np.inf
    _, got = _query(R, v, t, qn)
    bad = np.zeros(len(q), dtype=bool)
    bad[[3, 64, 200]] = True
    assert np.isnan(got[0][bad]).all() and np.isnan(got[1][bad]).all() and (got[2][bad] == -1).all()
    _same(tuple(x[~bad] for x in got), tuple(x[~bad] for x in clean), "neighbours of non-finite queries")
    # a triangle with an inf / NaN vertex is skipped and flagged; everything else is as without it
    for poison in (np.inf, np.nan):
        vp = np.concatenate([v, [[0.0, poison, 0.0]]])
        tp = np.concatenate([t, [[0, 1, len(v)]]]).astype(np.int32)
        for cells in (None, 3):
            index, got = _query(R, vp, tp, q, cells=cells)
            assert index.skipped and (got[2] < len(t)).all()
            _same(got, clean, f"a triangle with a {poison} vertex, cells={cells}")
    assert not R.MeshIndex(_dev(v), _dev(t)).skipped
    # an index outside [0, V)
    for wrong in (-1, len(v)):
        tw = t.copy()
        tw[17, 2] = wrong
        with pytest.raises(ValueError, match="index outside"):
            R.MeshIndex(_dev(v), _dev(tw))
        with pytest.raises(ValueError, match="index outside"):
            R.sample_surface(_dev(v), _dev(tw), 10)
    # no triangle / only skipped triangles: +inf, NaN, -1
    for vv, tt in ((v, np.zeros((0, 3), dtype=np.int32)), (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32)),
                   (np.full((3, 3), np.nan), np.array([[0, 1, 2]], dtype=np.int32))):
        index, got = _query(R, vv, tt, q)
        assert index.n_entries == 0 and np.isposinf(got[0]).all() and np.isnan(got[1]).all() and (got[2] == -1).all()
    # N = 0 and the sizes around a wavefront and a workgroup
    index, got = _query(R, v, t, np.zeros((0, 3)))
    assert got[0].shape == (0,) and got[1].shape == (0, 3) and got[2].shape == (0,)
    for n in (1, 63, 65, 257):
        _same(_query(R, v, t, q[:n])[1], tuple(x[:n] for x in clean), f"N = {n}")
    # float32 points, CPU points
    with pytest.raises(ValueError, match="float64"):
        index.closest(_dev(q.astype(np.float32)))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        index.closest(torch.from_numpy(q))


_spread_mesh = F.spread_mesh


def test_surface_samples(R):
    v, t, zero = _spread_mesh()
    area = F.triangle_areas(v, t)
    pos = area[area > 0]
    assert pos.max() / pos.min() > 1e6 and (area[zero] == 0.0).all() and len(pos) == len(t) - len(zero)
    n = 6000
    out = R.sample_surface(_dev(v), _dev(t), n, seed=3)
    pts, tri, bary, nrm = (out[k].cpu().numpy() for k in ("points", "triangle", "bary", "normal"))
    assert pts.shape == (n, 3) and tri.shape == (n,) and tri.dtype == np.int32 and bary.shape == (n, 3) and nrm.shape == (n, 3)
    assert abs(out["area"] - area.sum()) <= 1e-12 * area.sum()
    # the weights: exact, >= 0, sum 1; the mixer is the documented one
    assert (bary >= 0).all() and np.abs((bary[:, 0] + bary[:, 1]) + bary[:, 2] - 1.0).max() <= 4 * F.EPS
    for k in (0, 1, 2, 77, n - 1):
        assert tuple(bary[k]) == F.sample_bary(3, k), f"sample {k}: the weights are not those of the documented mixer"
    # the points: the convex combination of their triangle's corners, to 4 ulps of the largest corner coordinate
    corners = v[t[tri]]
    want = (bary[:, 0, None] * corners[:, 0] + bary[:, 1, None] * corners[:, 1]) + bary[:, 2, None] * corners[:, 2]
    scale = np.abs(corners).max(axis=(1, 2))
    assert (np.abs(pts - want).max(axis=1) <= 4 * F.EPS * scale).all()
    # the normals: unit, across both edges
    ln = np.sqrt((nrm * nrm).sum(axis=1))
    assert np.abs(ln - 1.0).max() <= 4 * F.EPS
    e1, e2 = corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]
    assert (np.abs((nrm * e1).sum(1)) <= 1e-12 * np.sqrt((e1 * e1).sum(1))).all() and ((nrm * np.cross(e1, e2)).sum(1) > 0).all()
    # area weighting: systematic sampling puts n A_t / A samples on triangle t, give or take the two ends of its interval
    counts = np.bincount(tri, minlength=len(t))
    dev_ = np.abs(counts - n * area / area.sum())
    print(f"surface samples: worst |c_t - n A_t / A| = {dev_.max():.3f}; {int((counts > 0).sum())} of {len(t)} triangles sampled")
    assert dev_.max() <= 2.0 and (counts[zero] == 0).all()
    # the same seed gives the same bits, another seed does not
    again = R.sample_surface(_dev(v), _dev(t), n, seed=3)
    other = R.sample_surface(_dev(v), _dev(t), n, seed=4)
    for k in ("points", "triangle", "bary", "normal"):
        assert torch.equal(again[k], out[k]), k
    assert not torch.equal(other["points"], out["points"]) and not torch.equal(other["bary"], out["bary"])
    # one triangle, 20,000 samples: uniform over it — each weight has mean 1/3 and variance 1/18
    v1, t1 = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 1.0], [0.5, 3.0, -1.0]]), np.array([[0, 1, 2]], dtype=np.int32)
    m = 20000
    one = R.sample_surface(_dev(v1), _dev(t1), m, seed=0)
    w = one["bary"].cpu().numpy()
    sigma = np.sqrt(1.0 / (18.0 * m))
    print(f"one triangle: mean weights - 1/3 = {(w.mean(axis=0) - 1 / 3) / sigma} sigma")
    assert (one["triangle"] == 0).all() and (np.abs(w.mean(axis=0) - 1.0 / 3.0) <= 4.0 * sigma).all()
    # n = 1, n = 0, nothing to sample
    single = R.sample_surface(_dev(v), _dev(t), 1, seed=9)
    assert single["points"].shape == (1, 3) and area[int(single["triangle"][0])] > 0
    assert R.sample_surface(_dev(v), _dev(t), 0)["points"].shape == (0, 3)
    with pytest.raises(ValueError, match="area"):
        R.sample_surface(_dev(v[:3] * 0.0), _dev(t[:1]), 5)
    with pytest.raises(ValueError, match="area"):
        R.sample_surface(_dev(v), _dev(t[:0]), 5)


def _sphere_mesh(R, n, r):
    """marching cubes of mc_shapes.sphere on the device, in model coordinates"""
    v, t = R.marching_cubes(_dev(mc_shapes.sphere(n, r=r, c=(0.0, 0.0, 0.0))), 0.0)
    return (v / (n - 1) * 2.0 - 1.0).contiguous(), t


def test_mesh_distance_statistics_are_those_of_the_reference_distances(R):
    va, ta = F.torus_mesh()
    vb, tb = (x.cpu().numpy() for x in _sphere_mesh(R, 12, 0.6))
    taus = (0.05, 0.15)
    out = R.mesh_distance(_dev(va), _dev(ta), _dev(vb), _dev(tb), n_samples=2000, thresholds=taus, seed=1, return_samples=True)
    pa, pb = out["samples_a"].cpu().numpy(), out["samples_b"].cpu().numpy()
    assert pa.shape == (2000, 3) and pb.shape == (2000, 3)
    da, db = np.sqrt(F.closest_all(pa, vb, tb)[0]), np.sqrt(F.closest_all(pb, va, ta)[0])
    # |sqrt(x) - sqrt(y)| <= sqrt|x - y|: a distance is within sqrt(bound) of the reference's; mean, rms and max move by
    # no more than their worst element does (+ the rounding of a 2,000-term sum)
    tol = np.sqrt(max(F.bound(pa, vb), F.bound(pb, va))) + 2000 * F.EPS * max(da.max(), db.max())
    assert np.abs(out["distance_a"].cpu().numpy() - da).max() <= tol and np.abs(out["distance_b"].cpu().numpy() - db).max() <= tol
    want = {"accuracy": da.mean(), "completeness": db.mean(), "chamfer": 0.5 * (da.mean() + db.mean()),
            "rms_accuracy": np.sqrt((da * da).mean()), "rms_completeness": np.sqrt((db * db).mean()),
            "max_accuracy": da.max(), "max_completeness": db.max(), "hausdorff": max(da.max(), db.max())}
    for k, w in want.items():
        assert isinstance(out[k], float) and abs(out[k] - w) <= tol, (k, out[k], w)
    assert out["accuracy"] > 0.05 and out["completeness"] > 0.05, "the two meshes are far apart: the statistics say something"
    for i, tau in enumerate(taus):
        assert min(np.abs(da - tau).min(), np.abs(db - tau).min()) > tol, "a reference distance sits on the threshold"
        p, r = (da < tau).mean(), (db < tau).mean()
        assert 0 < p < 1 and 0 < r < 1
        assert abs(out["precision"][i] - p) <= 1e-12 and abs(out["recall"][i] - r) <= 1e-12
        assert abs(out["fscore"][i] - 2 * p * r / (p + r)) <= 1e-12
    assert out["thresholds"] == taus


def test_mesh_distance_of_known_shapes(R):
    # a mesh against itself: every sample lies on it
    v, t = F.torus_mesh()
    out = R.mesh_distance(_dev(v), _dev(t), _dev(v), _dev(t), n_samples=3000, thresholds=(1e-6,), return_samples=True)
    tol = F.bound(v, v)
    assert float((out["distance_a"] ** 2).max()) <= tol and float((out["distance_b"] ** 2).max()) <= tol
    assert out["precision"] == (1.0,) and out["recall"] == (1.0,) and out["fscore"] == (1.0,) and out["chamfer"] <= np.sqrt(tol)
    # concentric spheres of radius 0.6 and 0.5: 0.1 apart, up to the chord error of marching cubes at this resolution
    n = 32
    h = 2.0 / (n - 1)
    (va, ta), (vb, tb) = _sphere_mesh(R, n, 0.6), _sphere_mesh(R, n, 0.5)
    out = R.mesh_distance(va, ta, vb, tb, n_samples=20000, thresholds=(0.05, 0.2))
    print(f"concentric spheres: {out}")
    assert abs(out["chamfer"] - 0.1) <= h * h / (8 * 0.5) + 1e-3
    assert abs(out["accuracy"] - 0.1) <= h * h / (8 * 0.5) + 1e-3 and abs(out["completeness"] - 0.1) <= h * h / (8 * 0.5) + 1e-3
    assert out["precision"] == (0.0, 1.0) and out["recall"] == (0.0, 1.0) and out["fscore"] == (0.0, 1.0)
    assert "samples_a" not in out and all(isinstance(out[k], float) for k in ("accuracy", "completeness", "chamfer", "hausdorff"))
