"""Host side of the mesh simplification (rnb_mesh_simplify_* of include/rnbneus.h, rnb_neus_fork_amd.mesh_simplify): the
symbols are declared, bound and exported together, the workspace query is a host function, every argument check comes
before anything touches a device, and the two formulations of the numpy reference the GPU tests compare against
(tests/mesh_simplify_ref.py) agree with each other and have the properties the definition promises.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rnb_neus_fork_amd as R
from oracle import mc_oracle as M
from tests import mesh_components_ref as F
from tests import mesh_simplify_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rnb_mesh_simplify_workspace_bytes", "rnb_mesh_simplify_count", "rnb_mesh_simplify_emit")
_MESH = {}


def _mesh(name):
    """(vertices, triangles) of volume A / the noise volume through the numpy marching cubes, once"""
    if name not in _MESH:
        _MESH[name] = M.marching_cubes({"A": F.volume_a, "noise": F.noise_volume}[name](), 0.0)
    return _MESH[name]


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
        # 64-bit sizes where the header says int64_t / size_t, a double for the cell size, pointers elsewhere
        for decl, ct in zip(m.group(1).split(","), argtypes):
            decl = decl.strip()
            if "*" in decl or decl.startswith("rnb_stream_t"):
                assert ct in (C.c_void_p, C.POINTER(C.c_int64)), (name, decl)
            elif decl.startswith("double"):
                assert ct is C.c_double, (name, decl)
            else:
                assert ct is (C.c_size_t if decl.startswith("size_t") else C.c_int64), (name, decl)
        assert hasattr(lib, name)
    assert lib.rnb_abi_version() == 5 and R.native.ABI_VERSION == 5
    from rnb_neus_fork_amd import buildid
    assert "mesh_simplify.hip" in buildid.HIP_SOURCES and "-ffp-contract=off" in buildid.EXTRA_FLAGS["mesh_simplify.hip"]
    assert "simplify_mesh" in R.__all__ and callable(R.simplify_mesh)


def _ws(V, T):
    b = C.c_int64(-7)
    return R.native.load().rnb_mesh_simplify_workspace_bytes(V, T, C.byref(b)), b.value


def test_workspace_query_is_monotone_and_refuses_bad_sizes():
    lib = R.native.load()
    sizes = [0, 1, 31, 32, 33, 255, 1024, 1025, 10 ** 6, 2 ** 30, 2 ** 30 + 1, 2 ** 31 - 1]
    table = np.array([[_ws(V, T) for T in sizes] for V in sizes])
    assert (table[:, :, 0] == 0).all()
    b = table[:, :, 1]
    assert (np.diff(b, axis=0) >= 0).all() and (np.diff(b, axis=1) >= 0).all()
    assert b[1, 0] > b[0, 0] and b[0, 1] > b[0, 0] and b[-1, 0] > b[-2, 0] > b[1, 0] and b[0, -1] > b[0, -2] > b[0, 1]
    # both tables hold at least two 4-byte slots per item, next to the per-vertex and per-triangle state
    V, T = 10 ** 6, 3 * 10 ** 6
    assert _ws(V, T)[1] >= 8 * V + 8 * T + 40 * V + 16 * T
    for V, T in ((-1, 0), (0, -1), (2 ** 31, 0), (0, 2 ** 31)):
        assert _ws(V, T) == (-1, -7), (V, T)                  # RNB_E_INVALID, nothing written
    assert lib.rnb_mesh_simplify_workspace_bytes(1, 1, None) == -4


def test_argument_checks_come_before_any_launch():
    """Every call below returns before a stream or the device is touched: the pointers are made up (a call that got as
    far as a launch would need a device), and a call with valid arguments stops at the NULL / short workspace."""
    lib = R.native.load()
    p = C.c_void_p(4096)           # never dereferenced on the host
    big = 1 << 40
    org = (C.c_double * 3)(0.0, 0.0, 0.0)
    nan, inf = float("nan"), float("inf")

    def count(V=8, T=4, verts=p, tri=p, origin=org, h=1.0, ws=p, wsb=big, counts=p):
        return lib.rnb_mesh_simplify_count(verts, V, tri, T, origin, h, ws, wsb, counts, None)

    def emit(V=8, T=4, verts=p, tri=p, origin=org, h=1.0, ws=p, wsb=big, nv=3, nt=1, vo=p, to=p, vi=p, vc=p, ti=p):
        return lib.rnb_mesh_simplify_emit(verts, V, tri, T, origin, h, ws, wsb, nv, nt, vo, to, vi, vc, ti, None)

    for call in (count, emit):
        assert call(V=-1) == -1 and call(T=-1) == -1 and call(V=2 ** 31) == -1 and call(T=2 ** 31) == -1
        for h in (0.0, -1.0, nan, inf):
            assert call(h=h) == -1, h
        assert b"cell_size" in lib.rnb_last_error_string()
        for d in range(3):
            for bad in (nan, inf, -inf):
                o = (C.c_double * 3)(0.0, 0.0, 0.0)
                o[d] = bad
                assert call(origin=o) == -1
        assert b"origin" in lib.rnb_last_error_string()
        assert call(verts=None) == -4 and call(tri=None) == -4
        assert call(ws=None) == -4 and b"workspace" in lib.rnb_last_error_string()
        assert call(wsb=8) == -2                                # RNB_E_WORKSPACE
        assert call(origin=None, wsb=8) == -2                   # the default origin is a valid argument
    assert count(counts=None) == -4
    assert emit(nv=9) == -1 and emit(nt=5) == -1 and emit(nv=-1) == -1 and emit(nt=-1) == -1
    assert emit(vo=None) == -4 and emit(to=None) == -4 and emit(vi=None) == -4
    assert emit(vc=None, ti=None, wsb=8) == -2                  # the two optional outputs may be NULL


def test_python_argument_checks_fire_on_the_host():
    v, t = (torch.from_numpy(x) for x in F.degenerate())
    for kw in ({}, {"cell_size": 1.0, "target_triangles": 10}):
        with pytest.raises(ValueError, match="exactly one"):
            R.simplify_mesh(v, t, **kw)
    for kw in ({"cell_size": 0.0}, {"cell_size": -1.0}, {"cell_size": float("nan")}, {"cell_size": float("inf")},
               {"cell_size": "2"}, {"target_triangles": 0}, {"target_triangles": 1.5}, {"target_triangles": -3}):
        with pytest.raises(ValueError, match="|".join(kw)):
            R.simplify_mesh(v, t, **kw)
    for bad in ((0.0, 1.0), (0.0, float("nan"), 0.0), (float("inf"), 0.0, 0.0)):
        with pytest.raises(ValueError, match="origin"):
            R.simplify_mesh(v, t, cell_size=1.0, origin=bad)
    for bad_t in (t.long(), t[:, :2], t.reshape(-1), t.numpy()):
        with pytest.raises(ValueError, match="triangles"):
            R.simplify_mesh(v, bad_t, cell_size=1.0)
    for bad_v in (v.float(), v[:, :2], v.reshape(-1), None):
        with pytest.raises(ValueError, match="vertices"):
            R.simplify_mesh(bad_v, t, cell_size=1.0)
    with pytest.raises(ValueError, match="attribute"):
        R.simplify_mesh(v, t, cell_size=1.0, attributes={"normals": torch.zeros(3, 3)})
    # valid arguments on CPU tensors: there is no CPU path
    for kw in ({"cell_size": 1.0}, {"target_triangles": 2}, {"target_triangles": 100},
               {"cell_size": 1.0, "origin": (0.0, 0.0, 0.0), "attributes": {"a": torch.zeros(len(v))}}):
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            R.simplify_mesh(v, t, **kw)
    # the renderer's `simplify` is a dict of simplify_mesh keywords, checked before the grid is evaluated
    from tests import mesh_attrs_util as U
    mc, p, _ = U.model("tiny")
    ren = R.build_from_named_params(mc, p, torch.device("cpu"))[3]
    assert ren.last_mesh_simplify is None
    for bad in ("small", {"cells": 2}, {}, {"cell_size": 0.0}, {"cell_size": 2.0, "target_triangles": 5},
                {"cell_size": 2.0, "attributes": {}}):
        with pytest.raises(ValueError, match="simplify|exactly one|cell_size"):
            ren.extract_geometry(U.LO, U.HI, 8, backend="native", simplify=bad)
        with pytest.raises(ValueError, match="simplify|exactly one|cell_size"):
            ren.extract_textured_geometry(U.LO, U.HI, 8, simplify=bad)


def _random_mesh(rng):
    """V <= 40, T <= 80; coordinates on a lattice of quarter cells (many on cell faces, many ties in d2), some off it;
    now and then a NaN / infinite / far vertex, an index out of range, an unreferenced vertex"""
    V, T = int(rng.integers(0, 41)), int(rng.integers(0, 81))
    v = rng.integers(-12, 13, (V, 3)).astype(np.float64) * 0.25
    off = rng.random(V) < 0.4
    v[off] += rng.standard_normal((int(off.sum()), 3)) * 0.3
    for bad in (np.nan, np.inf, 3.0e6, -3.0e6):
        if V and rng.random() < 0.15:
            v[rng.integers(0, V), rng.integers(0, 3)] = bad
    t = rng.integers(0, max(V, 1), (T, 3)).astype(np.int32)
    if T and rng.random() < 0.2:
        t[rng.integers(0, T), rng.integers(0, 3)] = rng.choice([-1, V, V + 7])
    if V == 0:
        t[:] = rng.integers(-2, 3, (T, 3))
    return v, t


def test_the_two_reference_formulations_agree():
    rng = np.random.default_rng(2024)
    seen_flags, n_dup, n_deg, n_neg = set(), 0, 0, 0
    for k in range(300):
        v, t = _random_mesh(rng)
        h = float(rng.choice([0.25, 0.5, 1.0, 1.5, 0.7]))
        origin = None if k % 3 == 0 else rng.choice([0.0, 0.5, -1.25, 2.0, 0.3], 3)
        a, b = S.simplify(v, t, h, origin), S.simplify_brute(v, t, h, origin)
        assert S.equal(a, b), (k, a["counts"], b["counts"])
        seen_flags.add(a["counts"][4])
        n_dup += a["counts"][3]
        n_deg += a["counts"][2]
        i, f, usable = S.cells(v, a["origin"], h)
        n_neg += int((i[usable] < 0).sum())
        assert ((f >= 0) & (f <= 1)).all()
    assert seen_flags == {0, 1, 2, 3} and n_dup > 50 and n_deg > 500 and n_neg > 500


def test_floor_not_truncation_and_cell_faces():
    v = np.array([[-0.5, 0.0, 0.0], [1.0, 0.0, 0.0], [0.999999, 0.0, 0.0], [-1.0, 2.0, 0.0]])
    i, f, usable = S.cells(v, (0.0, 0.0, 0.0), 1.0)
    assert usable.all() and i[:, 0].tolist() == [-1, 1, 0, -1] and f[:, 0].tolist() == [0.5, 0.0, 0.999999, 0.0]
    i, f, usable = S.cells(np.array([[2.0 ** 20 - 0.5, 0, 0], [2.0 ** 20, 0, 0], [-2.0 ** 20, 0, 0], [-2.0 ** 20 - 0.5, 0, 0]]),
                           (0.0, 0.0, 0.0), 1.0)
    assert usable.tolist() == [True, False, True, False]


@pytest.mark.parametrize("name,h", [("A", 1.5), ("A", 4.0), ("noise", 2.5)])
def test_reference_properties_on_the_marching_cubes_volumes(name, h):
    v, t = _mesh(name)
    out = S.simplify(v, t, h, origin=(-0.3, 0.2, 0.1))
    nv, nt, n_deg, n_dup, flags, n_clusters = out["counts"]
    assert flags == 0 and 0 < nt < len(t) and 0 < nv <= n_clusters < len(v)
    # every output vertex is an input vertex of its own cluster
    assert np.array_equal(out["vertices"], v[out["vertex_index"]])
    assert np.array_equal(out["vertex_cluster"][out["vertex_index"]], np.arange(nv))
    i, _, _ = S.cells(v, out["origin"], h)
    for j in np.random.default_rng(0).integers(0, nv, 50):
        mem = np.flatnonzero(out["vertex_cluster"] == j)
        assert (i[mem] == i[out["vertex_index"][j]]).all() and out["vertex_index"][j] in mem
    # no degenerate and no duplicate triangle
    to = out["triangles"]
    assert (to[:, 0] != to[:, 1]).all() and (to[:, 1] != to[:, 2]).all() and (to[:, 0] != to[:, 2]).all()
    assert len(np.unique(np.sort(to, axis=1), axis=0)) == nt
    assert nt + n_deg + n_dup == len(t)
    assert np.array_equal(out["vertex_cluster"][t[out["triangle_index"]]], to)
    assert (np.diff(out["triangle_index"]) > 0).all() and (np.diff(np.flatnonzero(out["vertex_cluster"] >= 0)[:1]) >= 0).all()


@pytest.mark.parametrize("name", ["A", "noise"])
def test_a_cell_below_the_vertex_spacing_is_the_cleanup_with_no_criteria(name):
    v, t = _mesh(name)
    h = 2.0 ** -12
    i, _, _ = S.cells(v, S.default_origin(v), h)
    assert len(np.unique(i, axis=0)) == len(v), "every vertex has a cell of its own"
    out = S.simplify(v, t, h)
    v1, t1, index, _, _ = F.clean(v, t)
    assert np.array_equal(out["vertices"], v1) and np.array_equal(out["triangles"], t1)
    assert np.array_equal(out["vertex_index"], index) and out["counts"] == [len(v1), len(t1), 0, 0, 0, len(v1)]
