"""Host side of the mesh evaluation (rnb_mesh_bins_*, rnb_mesh_closest_points, rnb_mesh_sample_* of include/rnbneus.h,
rnb_neus_fork_amd.mesh_eval): the numpy reference the GPU tests compare against (tests/mesh_distance_ref.py) agrees with
the analytic torus and with its own second formulation, the symbols are declared, bound and exported together, and every
argument check comes before anything touches a device.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rnb_neus_fork_amd as R
from tests import mesh_distance_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rnb_mesh_bins_workspace_bytes", "rnb_mesh_bins_count", "rnb_mesh_bins_emit", "rnb_mesh_closest_points",
           "rnb_mesh_sample_workspace_bytes", "rnb_mesh_sample_areas", "rnb_mesh_sample_surface")
OK, E_INVALID, E_WORKSPACE, E_NULL = 0, -1, -2, -4


def test_reference_against_the_analytic_torus_and_its_second_formulation():
    case = F.torus_case()
    v, t, q = case["vertices"], case["triangles"], case["queries"]
    assert v.shape == (600, 3) and t.shape == (1200, 3) and len(q) == 1500 + 600 + 1200 + 1200
    d2, cl, tr = case["ref"]
    # the mesh interpolates the torus on a grid of spacing h: its distance field is the torus's to within h
    h = 2.0 / (F.TORUS_N - 1)
    assert np.abs(np.sqrt(d2) - F.torus_distance(q)).max() < h
    assert np.abs(np.sqrt(d2) - F.torus_distance(q)).max() > 1e-4, "a mesh is not the torus: the comparison is not vacuous"
    # vertices are on the mesh, centroids too; 1e-9 off a face is 1e-9 away
    tol = F.bound(q, v)
    assert (d2[1500:1500 + 600] == 0.0).all() and (d2[2100:3300] <= tol).all()
    assert np.abs(d2[3300:] - 1e-18).max() <= tol and np.abs(np.sqrt(d2[3300:]) - 1e-9).max() < 1e-7
    # the two formulations, at the bound of the tolerance rule
    e2, ecl, etr = F.closest_all(q, v, t, fn=F.point_triangle_ericson)
    worst = np.abs(e2 - d2).max() / (F.EPS * (tol / (16 * F.EPS)))
    print(f"two formulations of the point-triangle distance: at most {worst:.3f} x 2^-52 L^2 apart; same triangle for "
          f"{(etr == tr).mean():.1%} of the queries")
    assert np.abs(e2 - d2).max() <= tol and not np.isnan(e2).any()
    assert np.abs(F.closest_all(case["far"], v, t, fn=F.point_triangle_ericson)[0] - case["ref_far"][0]).max() <= F.bound(case["far"], v)
    # the parity rule passes the reference and refuses what it is there to refuse
    F.check_closest("reference against itself", q, v, t, case["ref"], d2, tol)
    with pytest.raises(AssertionError, match="dist2"):
        F.check_closest("dist2 off", q, v, t, (d2 + 4 * tol, cl, tr), d2, tol)
    with pytest.raises(AssertionError, match="off its triangle"):
        F.check_closest("wrong triangle", q, v, t, (d2, cl, (tr + 600) % 1200), d2, tol)
    with pytest.raises(AssertionError, match="differs from dist2"):
        F.check_closest("wrong point", q, v, t, (d2, v[t[tr, 0]], tr), d2, tol)


def test_reference_on_degenerate_triangles_and_non_finite_input():
    a, b = np.array([0.25, -0.5, 0.125]), np.array([1.0, 0.75, -0.5])
    q = np.random.default_rng(5).uniform(-2.0, 2.0, (200, 3))
    ab = b - a
    s = np.clip(((q - a) @ ab) / (ab @ ab), 0.0, 1.0)
    seg = ((q - (a + s[:, None] * ab)) ** 2).sum(axis=1)
    tol = F.bound(q, np.stack([a, b]))
    for corners in ([a, a, b], [a, b, b], [b, a, a], [a, a + 0.25 * ab, b], [a, b, a + 0.5 * ab]):
        d2, cl, tr = F.closest_all(q, np.array(corners), [[0, 1, 2]])
        assert np.abs(d2 - seg).max() <= tol and (tr == 0).all()
    d2 = F.closest_all(q, np.array([a, a, a]), [[0, 1, 2]])[0]
    assert np.abs(d2 - ((q - a) ** 2).sum(axis=1)).max() <= tol
    # unusable triangles are skipped; non-finite queries and an empty mesh have their own answers
    v = np.array([a, b, [0.0, 1.0, 0.0], [np.inf, 0.0, 0.0]])
    t = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4], [-1, 1, 2]])
    assert F.usable(v, t).tolist() == [True, False, False, False]
    qn = q[:4].copy()
    qn[1, 2] = np.nan
    d2, cl, tr = F.closest_all(qn, v, t)
    assert tr.tolist() == [0, -1, 0, 0] and np.isnan(d2[1]) and np.isnan(cl[1]).all()
    assert np.array_equal(d2[[0, 2, 3]], F.closest_all(q[[0, 2, 3]], v[:3], t[:1])[0])
    d2, cl, tr = F.closest_all(q[:3], v, t[1:])
    assert np.isposinf(d2).all() and np.isnan(cl).all() and (tr == -1).all()
    assert F.triangle_areas(v, t).tolist()[1:] == [0.0, 0.0, 0.0] and F.triangle_areas(v, t)[0] > 0


def test_the_documented_mixer_samples_a_triangle_uniformly():
    header = open(os.path.join(ROOT, "include", "rnbneus.h")).read()
    for const in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB"):
        assert const in header, "the header spells the mixer out"
    assert F.mix(0) == 0xE220A8397B1DCDAF, "splitmix64's first output for seed 0"
    n = 20000
    for seed in (0, 1, 2 ** 64 - 1):
        w = np.array([F.sample_bary(seed, k) for k in range(n)])
        assert (w >= 0).all() and ((w[:, 0] + w[:, 1]) + w[:, 2] == 1.0).all()
        assert (np.abs(w.mean(axis=0) - 1 / 3) <= 4 * np.sqrt(1 / (18 * n))).all()
        assert 0.0 <= F.sample_offset(seed) < 1.0
    assert F.sample_bary(0, 5) != F.sample_bary(1, 5) and F.sample_bary(0, 5) != F.sample_bary(0, 6)


def test_symbols_are_declared_bound_and_exported():
    lib = R.native.load()
    header = open(os.path.join(ROOT, "include", "rnbneus.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMBOLS:
        assert name in R.native.EXPORTED_SYMBOLS
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/rnbneus.h"
        restype, argtypes = R.native._SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(m.group(1).split(",")), f"{name}: argument count"
        for decl, ct in zip(m.group(1).split(","), argtypes):
            decl = decl.strip()
            if "rnb_mesh_bins*" in decl:
                assert ct is C.POINTER(R.native.MeshBins), (name, decl)
            elif "*" in decl or decl.startswith("rnb_stream_t"):
                assert ct in (C.c_void_p, C.POINTER(C.c_int64)), (name, decl)
            else:
                want = {"size_t": C.c_size_t, "int64_t": C.c_int64, "int32_t": C.c_int32}[decl.split()[0]]
                assert ct is want, (name, decl)
        assert hasattr(lib, name)
    assert lib.rnb_abi_version() == 5 and R.native.ABI_VERSION == 5
    m = re.search(r"typedef struct rnb_mesh_bins \{(.*?)\}", header, flags=re.S)
    assert m and [f.split()[0] for f in m.group(1).split(";") if f.strip()] == ["double", "double", "int32_t", "int32_t"]
    assert C.sizeof(R.native.MeshBins) == 48
    from rnb_neus_fork_amd import buildid
    assert "mesh_eval.hip" in buildid.HIP_SOURCES and buildid.EXTRA_FLAGS["mesh_eval.hip"] == ["-ffp-contract=off"]
    assert {"MeshIndex", "sample_surface", "mesh_distance"} <= set(R.__all__)
    assert all(hasattr(R, n) for n in ("MeshIndex", "sample_surface", "mesh_distance"))


def _bins(dims=(4, 4, 4), cell=0.5, origin=(0.0, 0.0, 0.0)):
    return R.native.MeshBins((C.c_double * 3)(*origin), cell, (C.c_int32 * 3)(*dims), 0)


def test_workspace_queries():
    lib = R.native.load()

    def ws(fn, n):
        b = C.c_int64(-7)
        return fn(n, C.byref(b)), b.value

    sizes = [1, 2, 1023, 1024, 1025, 10 ** 6, 2 ** 24]
    got = [ws(lib.rnb_mesh_bins_workspace_bytes, n) for n in sizes]
    assert all(rc == OK for rc, _ in got) and np.all(np.diff([b for _, b in got]) >= 0)
    assert got[-1][1] >= 4 * 2 ** 24, "one cursor per cell"
    for n in (0, -1, 2 ** 24 + 1):
        assert ws(lib.rnb_mesh_bins_workspace_bytes, n) == (E_INVALID, -7)
    assert lib.rnb_mesh_bins_workspace_bytes(8, None) == E_NULL
    got = [ws(lib.rnb_mesh_sample_workspace_bytes, n) for n in [0, 1, 1024, 1025, 10 ** 7, 2 ** 31 - 1]]
    assert got[0] == (OK, 0) and all(rc == OK for rc, _ in got) and np.all(np.diff([b for _, b in got]) >= 0)
    for n in (-1, 2 ** 31):
        assert ws(lib.rnb_mesh_sample_workspace_bytes, n) == (E_INVALID, -7)
    assert lib.rnb_mesh_sample_workspace_bytes(8, None) == E_NULL


def test_argument_checks_come_before_any_launch():
    """Every call below returns before a stream or the device is touched: the pointers are made up (a call that got as
    far as a launch would need a device), and a call with valid arguments stops at the NULL / short workspace."""
    lib = R.native.load()
    p = C.c_void_p(4096)           # never dereferenced on the host
    big = 1 << 40
    good = _bins()
    bad_bins = [_bins(dims=(0, 4, 4)), _bins(dims=(4, -1, 4)), _bins(dims=(512, 512, 512)), _bins(cell=0.0), _bins(cell=-1.0),
                _bins(cell=float("nan")), _bins(cell=float("inf")), _bins(origin=(0.0, float("nan"), 0.0)),
                _bins(origin=(float("inf"), 0.0, 0.0)), _bins(origin=(1e308, 0.0, 0.0), cell=1e307, dims=(64, 1, 1))]

    def count(V=8, T=4, verts=p, tri=p, bins=good, ws=p, wsb=big, cs=p, counts=p):
        return lib.rnb_mesh_bins_count(verts, V, tri, T, C.byref(bins) if bins is not None else None, ws, wsb, cs, counts, None)

    assert count(V=-1) == E_INVALID and count(T=-1) == E_INVALID and count(V=2 ** 31) == E_INVALID and count(T=2 ** 31) == E_INVALID
    assert all(count(bins=b) == E_INVALID for b in bad_bins)
    assert count(bins=None) == E_NULL and count(verts=None) == E_NULL and count(tri=None) == E_NULL
    assert count(cs=None) == E_NULL and count(counts=None) == E_NULL
    assert count(ws=None) == E_NULL and b"workspace" in lib.rnb_last_error_string()
    assert count(wsb=8) == E_WORKSPACE

    def emit(V=8, T=4, verts=p, tri=p, bins=good, ws=p, wsb=big, cs=p, E=9, entries=p, corners=p):
        return lib.rnb_mesh_bins_emit(verts, V, tri, T, C.byref(bins) if bins is not None else None, ws, wsb, cs, E, entries,
                                      corners, None)

    assert emit(V=-1) == E_INVALID and emit(T=2 ** 31) == E_INVALID and emit(E=-1) == E_INVALID and emit(E=2 ** 31) == E_INVALID
    assert all(emit(bins=b) == E_INVALID for b in bad_bins)
    assert emit(bins=None) == E_NULL and emit(tri=None) == E_NULL and emit(cs=None) == E_NULL
    assert emit(entries=None) == E_NULL and emit(corners=None) == E_NULL and emit(ws=None) == E_NULL
    assert emit(wsb=8) == E_WORKSPACE
    assert emit(T=0, E=0, tri=None, verts=None, entries=None, corners=None) == OK          # nothing to emit, nothing launched

    def closest(q=p, N=5, bins=good, cs=p, entries=p, E=9, corners=p, T=4, flags=R.native.MESH_BINS_COVER, d2=p, cl=p, tr=p):
        return lib.rnb_mesh_closest_points(q, N, C.byref(bins) if bins is not None else None, cs, entries, E, corners, T, flags,
                                           d2, cl, tr, None)

    assert closest(N=-1) == E_INVALID and closest(N=2 ** 31) == E_INVALID and closest(E=-1) == E_INVALID and closest(T=-1) == E_INVALID
    assert closest(flags=2) == E_INVALID and closest(flags=-1) == E_INVALID and b"flag" in lib.rnb_last_error_string()
    assert all(closest(bins=b) == E_INVALID for b in bad_bins)
    assert closest(bins=None) == E_NULL and closest(q=None) == E_NULL and closest(cs=None) == E_NULL
    assert closest(entries=None) == E_NULL and closest(corners=None) == E_NULL
    assert closest(d2=None, cl=None, tr=None) == E_NULL
    assert closest(N=0, q=None) == OK                                                       # no query: nothing launched

    def areas(V=8, T=4, verts=p, tri=p, ws=p, wsb=big, cum=p, total=p):
        return lib.rnb_mesh_sample_areas(verts, V, tri, T, ws, wsb, cum, total, None)

    assert areas(V=-1) == E_INVALID and areas(T=2 ** 31) == E_INVALID
    assert areas(verts=None) == E_NULL and areas(tri=None) == E_NULL and areas(cum=None) == E_NULL and areas(total=None) == E_NULL
    assert areas(ws=None) == E_NULL and areas(wsb=8) == E_WORKSPACE

    def sample(V=8, T=4, verts=p, tri=p, cum=p, total=p, n=16, seed=0, pts=p, tr=p, bary=p, nrm=p):
        return lib.rnb_mesh_sample_surface(verts, V, tri, T, cum, total, n, seed, pts, tr, bary, nrm, None)

    assert sample(V=-1) == E_INVALID and sample(n=-1) == E_INVALID and sample(n=2 ** 31) == E_INVALID
    assert sample(T=0) == E_INVALID and b"without triangles" in lib.rnb_last_error_string()
    assert sample(verts=None) == E_NULL and sample(tri=None) == E_NULL and sample(cum=None) == E_NULL and sample(total=None) == E_NULL
    assert sample(pts=None, tr=None, bary=None, nrm=None) == E_NULL
    assert sample(n=0, verts=None) == OK                                                    # no sample: nothing launched


def test_python_argument_checks_fire_on_the_host():
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64)
    t = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    for bad_t in (t.long(), t[:, :2], t.reshape(-1), t.numpy()):
        with pytest.raises(ValueError, match="triangles"):
            R.MeshIndex(v, bad_t)
        with pytest.raises(ValueError, match="triangles"):
            R.sample_surface(v, bad_t, 4)
        with pytest.raises(ValueError, match="triangles"):
            R.mesh_distance(v, bad_t, v, t, n_samples=4)
    for bad_v in (v.float(), v[:, :2], v.reshape(-1)):
        with pytest.raises(ValueError, match="vertices"):
            R.MeshIndex(bad_v, t)
        with pytest.raises(ValueError, match="vertices"):
            R.sample_surface(bad_v, t, 4)
        with pytest.raises(ValueError, match="vertices"):
            R.mesh_distance(v, t, bad_v, t, n_samples=4)
    for cells in (0, -3, (2, 2), (2, 0, 2), 2.5, (1.0, 2, 2), 257, (4096, 4096, 2), True):
        with pytest.raises(ValueError, match="cells"):
            R.MeshIndex(v, t, cells=cells)
    for grid in (((0.0, 0.0), 1.0, (2, 2, 2)), ((0.0, 0.0, float("nan")), 1.0, (2, 2, 2)), ((0.0, 0.0, 0.0), 0.0, (2, 2, 2)),
                 ((0.0, 0.0, 0.0), 1.0, (2, 0, 2)), ((0.0, 0.0, 0.0), float("inf"), (2, 2, 2))):
        with pytest.raises(ValueError, match="grid|cells"):
            R.MeshIndex(v, t, grid=grid)
    with pytest.raises(ValueError, match="not both"):
        R.MeshIndex(v, t, cells=2, grid=((0.0, 0.0, 0.0), 1.0, (2, 2, 2)))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        R.MeshIndex(v, t, grid=((0.0, 0.0, 0.0), 1.0, (2, 2, 2)))
    for n in (-1, 2.5, 2 ** 31, True):
        with pytest.raises(ValueError, match="n must"):
            R.sample_surface(v, t, n)
    with pytest.raises(ValueError, match="seed"):
        R.sample_surface(v, t, 4, seed=0.5)
    for kw in ({"n_samples": 0}, {"n_samples": 1.5}, {"thresholds": (-0.1,)}, {"thresholds": (float("nan"),)}):
        with pytest.raises(ValueError, match="|".join(kw)):
            R.mesh_distance(v, t, v, t, **kw)
    # valid arguments on CPU tensors: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        R.MeshIndex(v, t)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        R.MeshIndex(v, t, cells=(2, 3, 4))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        R.sample_surface(v, t, 4)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        R.mesh_distance(v, t, v, t, n_samples=4)


def test_default_grid():
    from rnb_neus_fork_amd.mesh_eval import default_grid, forced_grid
    for ext, T in (((1.0, 1.0, 1.0), 1200), ((1.52, 1.52, 0.44), 1200), ((1.0, 0.01, 30.0), 1200), ((3.0, 0.0, 2.0), 5000),
                   ((0.0, 0.0, 7.0), 100), ((2.0, 2.0, 2.0), 10 ** 7), ((1.0, 1.0, 1.0), 10 ** 9), ((1e-3, 1e3, 1.0), 10 ** 9)):
        dims, cell = default_grid(ext, T)
        n = dims[0] * dims[1] * dims[2]
        assert all(d >= 1 for d in dims) and n <= 2 ** 24 and cell > 0
        assert all(d * cell > e for d, e in zip(dims, ext)), "the grid covers the box"
        target = min(max(T, 1) // 2, 2 ** 24)
        flat = sum(e < cell for e in ext)
        if flat == 0:
            assert target / 4 <= n <= 4 * target + 64, (ext, T, dims)
    assert default_grid((0.0, 0.0, 0.0), 100) == ((1, 1, 1), 1.0)
    assert default_grid((1.0, 2.0, 3.0), 0)[0] == (1, 1, 1) and default_grid((1.0, 2.0, 3.0), 3)[0] == (1, 1, 1)
    assert forced_grid((0.0, 0.0, 0.0), (2, 2, 2)) == 1.0
    cell = forced_grid((7.0, 3.0, 5.0), (7, 3, 5))
    assert 1.0 < cell < 1.0 + 1e-9
