"""Host side of the mesh cleanup (rnb_mesh_* of include/rnbneus.h, rnb_neus_fork_amd.mesh_clean): the symbols are declared,
bound and exported together, the workspace query is a host function, every argument check comes before anything touches a
device, and the numpy reference the GPU tests compare against (tests/mesh_components_ref.py) agrees with scipy and
reproduces the facts the GPU tests rely on.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rnb_neus_fork_amd as R
from oracle import mc_oracle as M
from tests import mesh_components_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rnb_mesh_clean_workspace_bytes", "rnb_mesh_components", "rnb_mesh_component_stats", "rnb_mesh_compact_count",
           "rnb_mesh_compact_emit")
_MESH = {}


def _mesh(name):
    """(vertices, triangles) of volume A / the big sphere alone / the noise volume through the numpy marching cubes, once"""
    if name not in _MESH:
        u = {"A": F.volume_a, "big": lambda: F.volume_a(spheres=F.A_SPHERES[:1]), "noise": F.noise_volume}[name]()
        _MESH[name] = M.marching_cubes(u, 0.0)
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
        # 64-bit sizes where the header says int64_t / size_t, pointers elsewhere
        for decl, ct in zip(m.group(1).split(","), argtypes):
            decl = decl.strip()
            if "*" in decl or decl.startswith("rnb_stream_t"):
                assert ct in (C.c_void_p, C.POINTER(C.c_int64)), (name, decl)
            else:
                assert ct is (C.c_size_t if decl.startswith("size_t") else C.c_int64), (name, decl)
        assert hasattr(lib, name)
    assert lib.rnb_abi_version() == 5 and R.native.ABI_VERSION == 5
    from rnb_neus_fork_amd import buildid
    assert "mesh_clean.hip" in buildid.HIP_SOURCES
    assert {"mesh_components", "clean_mesh"} <= set(R.__all__)


def _ws(V, T):
    b = C.c_int64(-7)
    return R.native.load().rnb_mesh_clean_workspace_bytes(V, T, C.byref(b)), b.value


def test_workspace_query_is_monotone_and_refuses_bad_sizes():
    lib = R.native.load()
    sizes = [0, 1, 255, 1024, 1025, 10 ** 6, 2 ** 31 - 1]
    table = np.array([[_ws(V, T) for T in sizes] for V in sizes])
    assert (table[:, :, 0] == 0).all()
    b = table[:, :, 1]
    assert (np.diff(b, axis=0) >= 0).all() and (np.diff(b, axis=1) >= 0).all()
    assert b[0, 0] == 0 and b[1, 0] > 0 and b[-1, 0] > b[1, 0] and b[0, -1] > b[0, 1] > 0
    # every stage fits: the old -> new map and both block-sum arrays (compaction), one byte + one word per vertex
    # (components), 20 bytes per possible component (statistics)
    V, T = 10 ** 6, 3 * 10 ** 6
    assert _ws(V, T)[1] >= max(4 * V + 4 * (V // 1024 + T // 1024), 5 * V, 20 * V)
    for V, T in ((-1, 0), (0, -1), (2 ** 31, 0), (0, 2 ** 31)):
        assert _ws(V, T) == (-1, -7), (V, T)                  # RNB_E_INVALID, nothing written
    assert lib.rnb_mesh_clean_workspace_bytes(1, 1, None) == -4


def test_argument_checks_come_before_any_launch():
    """Every call below returns before a stream or the device is touched: the pointers are made up (a call that got as
    far as a launch would need a device), and a call with valid arguments stops at the NULL / short workspace."""
    lib = R.native.load()
    p = C.c_void_p(4096)           # never dereferenced on the host
    big = 1 << 40

    def components(T=4, V=8, tri=p, ws=p, wsb=big, labels=p, counts=p):
        return lib.rnb_mesh_components(tri, T, V, ws, wsb, labels, counts, None)

    assert components(V=-1) == -1 and components(T=-1) == -1 and components(V=2 ** 31) == -1
    assert components(tri=None) == -4 and components(labels=None) == -4 and components(counts=None) == -4
    assert components(ws=None) == -4 and b"workspace" in lib.rnb_last_error_string()
    assert components(wsb=8) == -2                              # RNB_E_WORKSPACE

    def stats(T=4, V=8, Cn=2, tri=p, verts=p, labels=p, ws=p, wsb=big, tc=p, vc=p, area=p, lo=p, hi=p):
        return lib.rnb_mesh_component_stats(tri, T, verts, V, labels, Cn, ws, wsb, tc, vc, area, lo, hi, None)

    assert stats(V=-1) == -1 and stats(Cn=-1) == -1 and stats(Cn=9) == -1
    assert stats(Cn=0) == 0                                     # nothing to do, nothing launched
    assert stats(labels=None) == -4 and stats(tc=None) == -4 and stats(tri=None) == -4
    assert stats(area=None) == -4 and stats(hi=None) == -4      # coordinates given: the geometric outputs are required
    assert stats(ws=None) == -4 and stats(wsb=8) == -2

    def count(T=4, V=8, Cn=2, tri=p, labels=p, keep=p, ws=p, wsb=big, counts=p):
        return lib.rnb_mesh_compact_count(tri, T, V, labels, keep, Cn, ws, wsb, counts, None)

    assert count(T=-1) == -1 and count(Cn=9) == -1 and count(V=2 ** 31) == -1
    assert count(tri=None) == -4 and count(labels=None) == -4 and count(keep=None) == -4 and count(counts=None) == -4
    assert count(ws=None) == -4 and count(wsb=8) == -2

    def emit(T=4, V=8, Cn=2, tri=p, verts=p, labels=p, keep=p, ws=p, wsb=big, nv=3, nt=1, vo=p, to=p, vi=p):
        return lib.rnb_mesh_compact_emit(tri, T, verts, V, labels, keep, Cn, ws, wsb, nv, nt, vo, to, vi, None)

    assert emit(V=-1) == -1 and emit(nv=9) == -1 and emit(nt=5) == -1 and emit(nv=-1) == -1
    assert emit(vo=None) == -4 and emit(to=None) == -4 and emit(vi=None) == -4 and emit(keep=None) == -4
    assert emit(ws=None) == -4 and emit(wsb=8) == -2


def test_python_argument_checks_fire_on_the_host():
    v, t = (torch.from_numpy(x) for x in F.degenerate())
    for bad_t in (t.long(), t[:, :2], t.reshape(-1), t.numpy()):
        with pytest.raises(ValueError, match="triangles"):
            R.mesh_components(bad_t, vertices=v)
        with pytest.raises(ValueError, match="triangles"):
            R.clean_mesh(v, bad_t)
    for bad_v in (v.float(), v[:, :2], v.reshape(-1)):
        with pytest.raises(ValueError, match="vertices"):
            R.mesh_components(t, vertices=bad_v)
        with pytest.raises(ValueError, match="vertices"):
            R.clean_mesh(bad_v, t)
    with pytest.raises(ValueError, match="n_vertices"):
        R.mesh_components(t)
    with pytest.raises(ValueError, match="n_vertices"):
        R.mesh_components(t, n_vertices=5, vertices=v)
    with pytest.raises(ValueError):
        R.mesh_components(t, n_vertices=-1)
    for kw in ({"keep_largest": 0}, {"keep_largest": -2}, {"keep_largest": 1.5}, {"min_fraction": -0.1},
               {"min_fraction": 1.5}, {"min_fraction": float("nan")}, {"min_triangles": -1}, {"by": "volume"}):
        with pytest.raises(ValueError, match="|".join(kw)):
            R.clean_mesh(v, t, **kw)
    with pytest.raises(ValueError, match="coordinates"):
        R.clean_mesh(None, t, by="area", keep_largest=1)
    with pytest.raises(ValueError, match="attribute"):
        R.clean_mesh(v, t, attributes={"normals": torch.zeros(3, 3)})
    # valid arguments on CPU tensors: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        R.mesh_components(t, vertices=v)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        R.mesh_components(t, n_vertices=8)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        R.clean_mesh(v, t, keep_largest=1)
    # the renderer's `clean` is a dict of clean_mesh keywords, checked before the grid is evaluated
    from tests import mesh_attrs_util as U
    mc, p, _ = U.model("tiny")
    ren = R.build_from_named_params(mc, p, torch.device("cpu"))[3]
    assert ren.last_mesh_clean is None
    for bad in ("largest", {"keep": 1}, {"keep_largest": 0}, {"min_fraction": 2.0}, {"attributes": {}}):
        with pytest.raises(ValueError, match="clean"):
            ren.extract_geometry(U.LO, U.HI, 8, backend="native", clean=bad)
        with pytest.raises(ValueError, match="clean"):
            ren.extract_textured_geometry(U.LO, U.HI, 8, clean=bad)


def _scipy_labels(triangles, V):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]]])
    g = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(V, V))
    _, lab = connected_components(g, directed=False)
    # to the id rule: components of referenced vertices, numbered by their smallest vertex
    ref = np.zeros(V, dtype=bool)
    ref[t.reshape(-1)] = True
    first = np.full(lab.max() + 1 if V else 0, V, dtype=np.int64)
    np.minimum.at(first, lab[ref], np.flatnonzero(ref))
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return np.where(ref, rank[lab], -1).astype(np.int32), int((first < V).sum())


@pytest.mark.parametrize("name", ["A", "noise"] + sorted(F.SMALL_MESHES))
def test_reference_components_agree_with_scipy(name):
    v, t = _mesh(name) if name in ("A", "noise") else F.SMALL_MESHES[name]()
    labels, n = F.components(t, len(v))
    want, n_want = _scipy_labels(t, len(v))
    assert n == n_want and np.array_equal(labels, want)
    if name == "noise":     # the id rule under renumbering: still scipy's partition, numbered by the new smallest vertices
        perm = np.random.default_rng(1).permutation(len(v))
        v2, t2 = F.renumber(v, t, perm)
        l2, n2 = F.components(t2, len(v2))
        w2, _ = _scipy_labels(t2, len(v2))
        assert n2 == n and np.array_equal(l2, w2)
        assert np.array_equal(np.sort(np.bincount(l2)), np.sort(np.bincount(labels)))


def test_small_meshes_are_what_their_names_say():
    for order in ("ascending", "descending", "bitrev"):
        v, t = F.SMALL_MESHES["strip_" + order]()
        labels, n = F.components(t, len(v))
        assert n == 1 and len(t) == 2049 and len(v) == 2051 and (labels == 0).all()
    v, t = F.two_fans()
    assert F.components(t, len(v))[1] == 1
    for n in (1, 255, 256, 257, 1025):
        v, t = F.isolated(n)
        labels, c = F.components(t, len(v))
        assert c == n and np.array_equal(labels, np.arange(3 * n) // 3)
    v, t = F.degenerate()
    labels, c = F.components(t, len(v))
    assert c == 3 and labels.tolist() == [0, 0, 0, 1, 1, 2, 1, -1]
    assert F.stats(t, labels, c, v)["triangles"].tolist() == [3, 2, 1]
    v, t = F.with_unreferenced()
    labels, c = F.components(t, len(v))
    assert c == 7 and labels[0] == -1 and labels[10] == -1 and labels[-1] == -1 and (labels >= 0).sum() == 21


def test_volume_a_facts():
    v, t = _mesh("A")
    assert v.shape == (1858, 3) and t.shape == (3704, 3)
    labels, n = F.components(t, len(v))
    st = F.stats(t, labels, n, v)
    assert n == 3 and st["triangles"].tolist() == [2940, 560, 204]
    span = [(int(np.flatnonzero(labels == c).min()), int(np.flatnonzero(labels == c).max())) for c in range(3)]
    assert span[1] == (1472, 1857) and span[2] == (1554, 1846), "components 1 and 2 interleave in vertex index"
    # keeping the big sphere and compacting gives marching cubes of the big sphere's volume alone, bit for bit
    vb, tb = _mesh("big")
    for kw in ({"keep_largest": 1}, {"min_fraction": 0.5}, {"min_triangles": 561}, {"by": "triangles", "keep_largest": 1}):
        v1, t1, index, keep, _ = F.clean(v, t, **kw)
        assert keep.tolist() == [True, False, False]
        assert np.array_equal(v1, vb) and np.array_equal(t1, tb) and np.array_equal(v[index], v1)
    # no criteria: unchanged
    v0, t0, index, keep, _ = F.clean(v, t)
    assert np.array_equal(v0, v) and np.array_equal(t0, t) and np.array_equal(index, np.arange(len(v)))
    assert F.clean(v, t, keep_largest=2)[3].tolist() == [True, True, False]
    assert F.clean(v, t, min_triangles=205)[3].tolist() == [True, True, False]
    # bbox and area are those of the spheres
    spheres = [F.A_SPHERES[i] for i in (0, 2, 1)]             # (the third sphere's first vertex comes before the second's)
    assert np.allclose(st["area"] * (2 / 39) ** 2, [4 * np.pi * r * r for _, r in spheres], rtol=0.08)
    centre = (st["bbox_min"] + st["bbox_max"]) / 2 * (2 / 39) - 1
    assert np.abs(centre - np.array([c for c, _ in spheres])).max() < 0.03


def test_noise_volume_facts_and_the_selection_rules():
    v, t = _mesh("noise")
    assert v.shape == (49436, 3) and t.shape == (103784, 3)
    labels, n = F.components(t, len(v))
    assert n == 370
    st = F.stats(t, labels, n, v)
    tc = st["triangles"]
    assert tc.sum() == len(t) and st["vertices"].sum() == len(v) and len(np.unique(tc)) < n, "ties in triangle count"
    # keep_largest: ties go to the smaller id
    k = 40
    keep = F.select(tc, tc, keep_largest=k)
    assert keep.sum() == k
    cut = np.sort(tc)[-k]
    assert (tc[keep] >= cut).all() and (tc[~keep] <= cut).all()
    tied_in, tied_out = np.flatnonzero(keep & (tc == cut)), np.flatnonzero(~keep & (tc == cut))
    assert len(tied_out) > 0 and len(tied_in) > 0 and tied_in.max() < tied_out.min()
    # NaN ranks below every number and passes no min_fraction; the criteria are ANDed
    m = np.array([3.0, np.nan, 5.0, 5.0, 1.0])
    n_t = np.array([10, 99, 2, 7, 7])
    assert F.select(m, n_t, keep_largest=2).tolist() == [False, False, True, True, False]
    assert F.select(m, n_t, keep_largest=5).tolist() == [True] * 5
    assert F.select(m, n_t, min_fraction=0.6).tolist() == [True, False, True, True, False]
    assert F.select(m, n_t, min_fraction=0.0).tolist() == [True, False, True, True, True]
    assert F.select(m, n_t, keep_largest=3, min_triangles=7).tolist() == [True, False, False, True, False]
    # the package's selection is the same rule (torch on the CPU here; the device runs the same ops)
    from rnb_neus_fork_amd.mesh_clean import select_components
    for kw in ({"keep_largest": 2}, {"min_fraction": 0.6}, {"min_fraction": 0.0}, {"keep_largest": 3, "min_triangles": 7}, {}):
        got = select_components(torch.from_numpy(m), torch.from_numpy(n_t), **kw)
        assert got.tolist() == F.select(m, n_t, **kw).tolist(), kw
    got = select_components(torch.from_numpy(tc), torch.from_numpy(tc), keep_largest=k)
    assert np.array_equal(got.numpy(), keep)
    # the area bound tells a dropped triangle from rounding: one triangle of the largest component is far outside it
    bound = F.area_bound(v, t, labels, n)
    big = int(np.argmax(tc))
    one = F.triangle_areas(v, t[labels[t[:, 0]] == big][:1])[0]
    assert one > 1e4 * bound[big] > 0
