"""Host side of the mesh topology audit (rnb_mesh_topology_* of include/rnbneus.h, rnb_neus_fork_amd.mesh_topology): the
two formulations of the numpy reference the GPU tests compare against (tests/mesh_topology_ref.py) agree with each other
and give the closed forms of shapes whose topology is known; the symbols are declared, bound and exported together, the
workspace query is a host function, and every argument check comes before anything touches a device.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rnb_neus_fork_amd as R
from tests import mesh_topology_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rnb_mesh_topology_workspace_bytes", "rnb_mesh_topology_count", "rnb_mesh_topology_emit",
           "rnb_mesh_topology_components")


def _random_mesh(rng):
    """V <= 30, T <= 70 with repeated, degenerate and now and then out-of-range indices"""
    V, T = int(rng.integers(0, 31)), int(rng.integers(0, 71))
    t = rng.integers(0, max(V, 1), (T, 3)).astype(np.int32)
    if T and rng.random() < 0.3:
        t[rng.integers(0, T), rng.integers(0, 3)] = rng.choice([-1, V, V + 5])
    if V == 0:
        t[:] = rng.integers(-2, 3, (T, 3))
    v = rng.standard_normal((V, 3))
    if V and rng.random() < 0.2:
        v[rng.integers(0, V), rng.integers(0, 3)] = rng.choice([np.nan, np.inf])
    return v, t


def test_the_two_reference_formulations_agree():
    shapes = dict(M.small_shapes())
    shapes["degenerate input"] = M.degenerate_input()
    shapes["no triangle"] = (np.zeros((5, 3)), np.zeros((0, 3), dtype=np.int32))
    shapes["no vertex"] = (np.zeros((0, 3)), np.array([[0, 1, 2], [0, 0, 0]], dtype=np.int32))
    shapes["fan"] = M.fan(50, mixed=True)
    for n in (1, 2, 85, 86):
        shapes[f"strip {n}"] = M.strip(n)
    for name, (v, t) in shapes.items():
        assert M.equal(M.topology(t, len(v), v), M.topology_brute(t, len(v), v)) is None, name
    rng = np.random.default_rng(7)
    classes, n_nan = np.zeros(5, dtype=np.int64), 0
    for k in range(200):
        v, t = _random_mesh(rng)
        a, b = M.topology(t, len(v), v), M.topology_brute(t, len(v), v)
        assert M.equal(a, b) is None, (k, M.equal(a, b))
        classes += a["counts"][1:6] > 0
        n_nan += int(np.isnan(a["volume"]).any())
        assert a["counts"][1:5].sum() == a["counts"][0] and np.array_equal(a["table"][:, :4].sum(axis=0), a["counts"][1:5])
    assert (classes > 20).all() and n_nan > 5, (classes, n_nan)


def _one(v, t):
    out = M.topology(t, len(v), v)
    assert out["n_components"] == 1
    return out


def test_closed_forms():
    out = _one(*M.tetrahedron())
    assert out["counts"].tolist() == [6, 0, 6, 0, 0, 0, 0, 0] and out["euler"][0] == 2 and out["genus"][0] == 0 and out["closed"][0]
    assert out["volume"][0] == pytest.approx(1 / 6, rel=1e-15)
    out = _one(*M.cube())
    assert out["closed"][0] and out["euler"][0] == 2 and out["volume"][0] == 1.0
    out = _one(*M.torus_grid(8, 6))
    assert out["closed"][0] and out["euler"][0] == 0 and out["genus"][0] == 1 and out["counts"][0] == 3 * 48
    out = _one(*M.cube(open_top=True))
    assert out["counts"][1] == 4 and out["counts"][7] == 1 and out["boundary_simple"] and out["euler"][0] == 1
    assert out["genus"][0] == 0 and not out["closed"][0] and out["table"][0, 6] == 1
    assert sorted(np.flatnonzero(out["boundary_labels"] == 0).tolist()) == [4, 5, 6, 7]
    out = _one(*M.shared_edge_tetrahedra())
    assert out["counts"][4] == 1 and out["edge_use"][(out["edge_use"].sum(axis=1) == 4)].tolist() == [[2, 2]] and out["genus"][0] == -1
    out = _one(*M.icosphere_one_reversed())
    assert out["counts"][3] == 3 and out["counts"][1] == 0 and not out["closed"][0]
    out = _one(*M.bow_tie())
    assert not out["boundary_simple"] and out["boundary_degree"][0] == 4 and out["counts"][7] == 1 and out["genus"][0] == -1
    assert (out["vertex_flags"] == 1).all(), "a bow-tie vertex has only boundary edges: not detected as such"
    v, t = M.fan(1000)
    out = _one(v, t)
    assert out["edge_use"][0].tolist() == [1000, 0] and out["counts"][4] == 1 and out["counts"][1] == 2000


def test_a_moebius_strip_has_a_flipped_edge_however_it_is_oriented():
    v, t = M.moebius()
    rng = np.random.default_rng(3)
    for k in range(40):
        tt = t.copy()
        flip = rng.random(len(t)) < 0.5 if k else np.zeros(len(t), dtype=bool)
        tt[flip] = tt[flip][:, ::-1]
        out = M.topology(tt, len(v))
        assert out["counts"][3] >= 1 and out["counts"][7] == 1 and out["counts"][4] == 0 and out["boundary_simple"]
        assert out["euler"][0] == 0


def test_icosphere_volume_and_its_sign():
    v, t = M.icosphere(3)
    want = M.polyhedral_volume(v, t)
    assert 0.97 * 4 / 3 * np.pi < want < 4 / 3 * np.pi
    out, rev = M.topology(t, len(v), v), M.topology(t[:, ::-1], len(v), v)
    assert out["closed"][0] and out["euler"][0] == 2
    assert abs(out["volume"][0] - want) <= 1e-12 * want and abs(rev["volume"][0] + want) <= 1e-12 * want
    assert out["volume_bound"][0] < 1e-13 * want


def test_the_large_torus_with_holes_is_neither_trivial_case():
    """the removed set of tests/test_gpu_mesh_topology.py's large case: between 100 and 1,000 boundary components"""
    v, t = M.torus_with_holes()
    assert len(t) == 359000
    out = M.topology(t, len(v))
    assert 100 <= out["counts"][7] <= 1000 and 0 < out["counts"][1] < out["counts"][0] // 100, out["counts"]
    assert out["n_components"] == 1 and out["table"][0, 6] == out["counts"][7]


def test_symbols_are_declared_bound_and_exported():
    lib = R.native.load()
    header = open(os.path.join(ROOT, "include", "rnbneus.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMBOLS:
        assert name in R.native.EXPORTED_SYMBOLS
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/rnbneus.h"
        restype, argtypes = R.native.signature(name)
        assert restype is C.c_int and len(argtypes) == len(m.group(1).split(",")), f"{name}: argument count"
        for decl, ct in zip(m.group(1).split(","), argtypes):
            decl = decl.strip()
            if "*" in decl or decl.startswith("rnb_stream_t"):
                assert ct in (C.c_void_p, C.POINTER(C.c_int64)), (name, decl)
            else:
                assert ct is (C.c_size_t if decl.startswith("size_t") else C.c_int64), (name, decl)
        assert hasattr(lib, name)
    assert lib.rnb_abi_version() == 5 and R.native.ABI_VERSION == 5
    from rnb_neus_fork_amd import buildid
    assert "mesh_topology.hip" in buildid.HIP_SOURCES and "-ffp-contract=off" in buildid.EXTRA_FLAGS["mesh_topology.hip"]
    names = [n for n, _ in buildid.source_files()]
    assert "csrc/mesh_table.hip.h" in names and "csrc/union_find.hip.h" in names, "the shared headers are hashed into the build id"
    for name in ("mesh_topology", "watertight"):
        assert name in R.__all__ and callable(getattr(R, name))


def _ws(V, T):
    b = C.c_int64(-7)
    return R.native.load().rnb_mesh_topology_workspace_bytes(V, T, C.byref(b)), b.value


def test_workspace_query_is_a_host_function():
    lib = R.native.load()
    sizes = [0, 1, 85, 86, 1024, 1025, 10 ** 6, 2 ** 30]
    table = np.array([[_ws(V, T) for T in sizes] for V in sizes])
    assert (table[:, :, 0] == 0).all()
    b = table[:, :, 1]
    assert (b > 0).all() and (np.diff(b, axis=0) >= 0).all() and (np.diff(b, axis=1) >= 0).all()
    # per half-edge the key, the leader, the two use counts and at least two 4-byte slots
    V, T = 10 ** 6, 2 * 10 ** 6
    assert _ws(V, T)[1] >= 3 * T * (8 + 4 + 4 + 4 + 8)
    for V, T in ((-1, 0), (0, -1), (2 ** 31, 0), (0, 1431655765), (0, 2 ** 31 - 1)):
        assert _ws(V, T) == (-1, -7), (V, T)                  # RNB_E_INVALID, nothing written
    assert _ws(2 ** 31 - 1, 1431655764)[0] == 0
    assert lib.rnb_mesh_topology_workspace_bytes(1, 1, None) == -4
    # native.workspace reaches it and applies the floor
    N, a = R.native, (1000, 2000)
    need = _ws(*a)[1]
    assert N.workspace_bytes("mesh_topology", *a) == need and N.workspace_bytes("mesh_topology", *a, floor=need + 3) == need + 3
    ws = N.workspace("mesh_topology", "cpu", *a)
    assert ws.dtype == torch.uint8 and ws.dim() == 1 and ws.numel() == need
    assert N.workspace("mesh_topology", "cpu", *a, floor=need + 17).numel() == need + 17
    assert N.workspace("mesh_topology", "cpu", *a, floor=need - 1).numel() == need
    with pytest.raises(N.NativeError):      # the return code is checked
        N.workspace("mesh_topology", "cpu", -7, 0)


def test_argument_checks_come_before_any_launch():
    """Every call below returns before a stream or the device is touched: the pointers are made up (a call that got as
    far as a launch would need a device), and a call with valid arguments stops at the NULL / short workspace."""
    lib = R.native.load()
    p = C.c_void_p(4096)           # never dereferenced on the host
    big = 1 << 40

    def count(T=4, V=8, tri=p, ws=p, wsb=big, counts=p, tf=p, vf=p, bl=p, bd=p):
        return lib.rnb_mesh_topology_count(tri, T, V, ws, wsb, counts, tf, vf, bl, bd, None)

    def emit(T=4, V=8, tri=p, ws=p, wsb=big, E=3, e=p, u=p, et=p):
        return lib.rnb_mesh_topology_emit(tri, T, V, ws, wsb, E, e, u, et, None)

    def comps(T=4, V=8, tri=p, verts=p, labels=p, C_=2, ws=p, wsb=big, table=p, vol=p):
        return lib.rnb_mesh_topology_components(tri, T, verts, V, labels, C_, ws, wsb, table, vol, None)

    for call in (count, emit, comps):
        assert call(V=-1) == -1 and call(T=-1) == -1 and call(V=2 ** 31) == -1 and call(T=2 ** 31 - 1) == -1
        assert b"half-edges" in lib.rnb_last_error_string()
        assert call(tri=None) == -4
        assert call(ws=None) == -4 and b"workspace" in lib.rnb_last_error_string()
        assert call(wsb=8) == -2                                # RNB_E_WORKSPACE
    exact = _ws(8, 4)[1]
    assert count(wsb=exact - 1) == -2 and emit(wsb=exact - 1) == -2 and comps(wsb=exact - 1) == -2
    assert count(counts=None) == -4 and count(tf=None) == -4 and count(vf=None) == -4
    assert count(bl=None) == -4 and count(bd=None) == -4 and b"come together" in lib.rnb_last_error_string()
    assert count(bl=None, bd=None, wsb=8) == -2                # both NULL is a valid argument: no boundary components
    assert emit(E=-1) == -1 and emit(E=13) == -1
    assert emit(e=None) == -4 and emit(u=None) == -4 and emit(et=None) == -4
    assert comps(C_=-1) == -1 and comps(C_=9) == -1
    assert comps(labels=None) == -4 and comps(table=None) == -4 and comps(vol=None) == -4
    assert comps(verts=None, vol=None, wsb=8) == -2            # no coordinates: no volume


def test_python_argument_checks_fire_on_the_host():
    v, t = (torch.from_numpy(x) for x in M.tetrahedron())
    for bad_t in (t.long(), t[:, :2], t.reshape(-1), t.numpy()):
        with pytest.raises(ValueError, match="triangles"):
            R.mesh_topology(bad_t, 4)
    for bad_v in (v.float(), v[:, :2], v.reshape(-1)):
        with pytest.raises(ValueError, match="vertices"):
            R.mesh_topology(t, vertices=bad_v)
    with pytest.raises(ValueError, match="n_vertices"):
        R.mesh_topology(t)
    with pytest.raises(ValueError, match="n_vertices"):
        R.mesh_topology(t, 5, v)
    with pytest.raises(ValueError, match="outside"):
        R.mesh_topology(t, -1)
    for kw in ({}, {"edges": True}, {"boundary": False, "components": False}):
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            R.mesh_topology(t, 4, **kw)
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            R.mesh_topology(t, vertices=v, **kw)
    with pytest.raises(ValueError, match="components"):
        R.watertight({"n_invalid": 0})
    import rnb_neus_fork_amd.mesh_pipeline as MP
    assert not any("topology" in str(row) for row in MP.STAGES), "the audit transforms nothing: it is no stage of the chain"
