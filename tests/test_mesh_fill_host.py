"""Host side of the hole filling: the numpy reference of tests/mesh_fill_ref.py against facts — the audit of
tests/mesh_topology_ref.py on the filled mesh, closed forms for the volumes — so that the GPU tests compare against something
that has itself been checked; then the argument checks of the Python layer and of the library (which return before any
launch), the `fill=` option of the extract calls, and the bindings.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import rnb_neus_fork_amd as R
from rnb_neus_fork_amd import mesh_pipeline as P
from tests import mesh_fill_ref as F
from tests import mesh_topology_ref as M


def _audit(v, t):
    return M.topology(t, len(v), v)


def _filled(mesh, **kw):
    """(reference fill, audit before, audit after) with the facts every fill obeys asserted"""
    v, t = mesh
    out = F.fill(v, t, **kw)
    before, after = _audit(v, t), _audit(out["vertices"], out["triangles"])
    n = out["info"]["n_filled"]
    if before["counts"][6] == 0:        # (an invalid triangle may come to name a new vertex: see the degenerate input below)
        assert F.euler_sum(after) - F.euler_sum(before) == n, "every filled loop raises the Euler characteristic by one"
        assert after["counts"][3] == before["counts"][3] and after["counts"][4] == before["counts"][4], "no flipped / non-manifold edge added"
        assert after["counts"][7] == before["counts"][7] - n
    assert np.array_equal(out["vertices"][:len(v)], v) and np.array_equal(out["triangles"][:len(t)], t)
    assert len(out["vertices"]) == len(v) + n and len(out["triangles"]) == len(t) + out["info"]["n_new_triangles"]
    return out, before, after


def test_open_cube_and_open_tetrahedron_close_with_their_volumes():
    out, before, after = _filled(M.cube(open_top=True))
    assert out["info"] == dict(zip(F.INFO_KEYS, (1, 1, 0, 0, 0, 4, 4)))
    assert not before["closed"].any() and after["closed"].all() and after["volume"][0] == 1.0
    assert out["loops"]["loop_vertices"].tolist() == [4, 6, 7, 5] and out["vertices"][8].tolist() == [0.5, 0.5, 1.0]
    # the side faces use the rim as 4 -> 6 -> 7 -> 5 (against the missing top (4, 5, 7, 6)); the cap runs against them
    assert out["triangles"][-4:].tolist() == [[6, 4, 8], [7, 6, 8], [5, 7, 8], [4, 5, 8]]
    out, _, after = _filled(F.open_tetrahedron())
    assert out["info"]["n_filled"] == 1 and out["info"]["longest_filled"] == 3 and after["closed"].all()
    assert abs(after["volume"][0] - 1 / 6) <= 2 ** -52
    assert out["loops"]["loop_vertices"].tolist() == [0, 2, 3], "the removed face (0, 3, 2), walked against it"


@pytest.mark.parametrize("n", [3, 63, 64, 65, 1025, -65])
def test_tubes_close_with_the_prism_volume(n):
    mesh = F.tube(abs(n))
    if n < 0:
        mesh = M.interleave([mesh], seed=3)
    n = abs(n)
    out, before, after = _filled(mesh)
    assert out["info"] == dict(zip(F.INFO_KEYS, (2, 2, 0, 0, 0, 2 * n, n)))
    assert F.euler_sum(before) == 0 and F.euler_sum(after) == 2 and after["closed"].all()
    assert abs(after["volume"][0] - 2 * F.ngon_area(n)) <= 1e-12 * n
    lp = out["loops"]
    assert lp["loop_edges"].tolist() == [n, n] and lp["loop_offsets"].tolist() == [0, n, 2 * n]
    assert (lp["loop_vertices"][[0, n]] == [lp["loop_vertices"][:n].min(), lp["loop_vertices"][n:].min()]).all()
    # inside out: the caps keep the sign
    v, t = F.inside_out(mesh)
    flipped = F.fill(v, t)
    a = _audit(flipped["vertices"], flipped["triangles"])
    assert a["closed"].all() and abs(a["volume"][0] + 2 * F.ngon_area(n)) <= 1e-12 * n


def test_loops_that_are_not_walked():
    out, _, _ = _filled(M.moebius())
    assert out["info"] == dict(zip(F.INFO_KEYS, (1, 0, 0, 1, 0, 0, 0))) and out["loops"]["loop_status"].tolist() == [F.MISORIENTED]
    assert out["loops"]["loop_vertices"].tolist() == sorted(out["loops"]["loop_vertices"].tolist())
    out, _, _ = _filled(M.bow_tie())
    assert out["info"] == dict(zip(F.INFO_KEYS, (1, 0, 1, 0, 0, 0, 0))) and out["loops"]["loop_status"].tolist() == [F.TANGLED]
    assert out["loops"]["loop_vertices"].tolist() == [0, 1, 2, 3, 4] and out["loops"]["loop_edges"].tolist() == [6]
    out, _, _ = _filled(M.small_shapes()["all interleaved"])
    assert out["info"]["n_loops"] == 3 and out["info"]["n_filled"] == 1
    assert sorted(out["loops"]["loop_status"].tolist()) == [F.SIMPLE, F.TANGLED, F.MISORIENTED]


def test_torus_with_holes():
    out, before, after = _filled(M.torus_with_holes(60, 30, 100))
    assert (out["info"]["n_loops"], out["info"]["n_filled"]) == (86, 76)
    assert (before["counts"][1], after["counts"][1]) == (294, 64)
    assert out["info"]["n_tangled"] == 10 and out["info"]["n_misoriented"] == 0
    limited = F.fill(*M.torus_with_holes(60, 30, 100), max_edges=3)
    assert 0 < limited["info"]["n_filled"] < 76 and limited["info"]["n_too_long"] == 76 - limited["info"]["n_filled"]
    assert limited["info"]["longest_filled"] == 3


def test_punched_sheet_and_attributes():
    m, k, q = 12, 12, 5
    mesh = F.punched_sheet(m, k, q)
    out, _, _ = _filled(mesh, max_edges=4)
    holes = F.punched_holes(m, k, q)
    assert holes > 5 and out["info"]["n_filled"] == holes and out["info"]["n_too_long"] == 1 and out["info"]["longest_filled"] == 4
    a = np.random.default_rng(2).normal(size=(len(mesh[0]), 5)).astype(np.float32)
    with_a = F.fill(*mesh, max_edges=4, attributes=a)
    assert with_a["attributes"].dtype == np.float32 and np.array_equal(with_a["attributes"][:len(a)], a)
    l = int(with_a["filled"][0])
    w = with_a["loops"]["_members"][l]
    assert np.allclose(with_a["attributes"][len(a)], a[w].astype(np.float64).mean(axis=0), rtol=1e-6)
    with pytest.raises(AssertionError, match="touch"):
        F.punched_sheet(10, 10, 3)


def test_degenerate_input_passes_through():
    """the old arrays come first bit for bit.  One consequence of copying invalid triangles as they are: (0, 1, 12) names
    index V = 12, and after the fill that is the first new vertex — the triangle has become proper.  The facts about the
    audit of a filled mesh therefore hold for inputs without invalid triangles, which is how `_filled` asserts them."""
    v, t = M.degenerate_input()
    out, before, after = _filled((v, t))
    assert np.array_equal(out["triangles"][:len(t)], t) and out["vertices"][:len(v)].tobytes() == v.tobytes()
    assert out["info"] == dict(zip(F.INFO_KEYS, (2, 1, 1, 0, 0, 3, 3)))
    # the lone triangle (0, 9, 8) is walked; the duplicate of (0, 5, 4) leaves the rim's vertices 4 and 5 with one boundary edge
    assert out["loops"]["loop_vertices"].tolist() == [0, 9, 8, 4, 5, 6, 7] and out["loops"]["loop_status"].tolist() == [0, 1]
    assert (before["counts"][6], after["counts"][6]) == (2, 1)


def test_python_argument_checks_fire_on_the_host():
    v, t = (torch.from_numpy(x) for x in M.tetrahedron())
    for bad_t in (t.long(), t[:, :2], t.reshape(-1), t.numpy()):
        with pytest.raises(ValueError, match="triangles"):
            R.boundary_loops(bad_t, 4)
        with pytest.raises(ValueError, match="triangles"):
            R.fill_holes(v, bad_t)
    for bad_v in (v.float(), v[:, :2], v.reshape(-1)):
        with pytest.raises(ValueError, match="vertices"):
            R.boundary_loops(t, vertices=bad_v)
        with pytest.raises(ValueError, match="vertices"):
            R.fill_holes(bad_v, t)
    with pytest.raises(ValueError, match="vertices is None"):
        R.fill_holes(None, t)
    with pytest.raises(ValueError, match="n_vertices"):
        R.boundary_loops(t)
    for bad in (2, 0, -1, 3.0, True, "4"):
        with pytest.raises(ValueError, match="max_edges"):
            R.fill_holes(v, t, max_edges=bad)
    with pytest.raises(ValueError, match="first dimension"):
        R.fill_holes(v, t, attributes={"a": torch.zeros(3, 2)})
    with pytest.raises(ValueError, match="float32"):
        R.fill_holes(v, t, attributes={"a": torch.zeros(4, 2, dtype=torch.uint8)})
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        R.boundary_loops(t, 4)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        R.fill_holes(v, t, max_edges=3, attributes={"a": torch.zeros(4, 2)})


def test_the_fill_option_of_the_extract_calls():
    P.check_options(fill=None)
    P.check_options(fill={})
    P.check_options(fill={"max_edges": 8})
    said = "fill must be a dict of fill_holes keywords ('max_edges',)"
    for bad in ({"max_edge": 8}, 8, [("max_edges", 8)], {"max_edges": 8, "attributes": {}}):
        with pytest.raises(ValueError) as e:
            P.check_options(fill=bad)
        assert str(e.value) == said
    with pytest.raises(ValueError, match="^fill: max_edges must be an integer >= 3"):
        P.check_options(fill={"max_edges": 2})
    assert tuple(s.name for s in P.STAGES) == ("clean", "cull", "simplify") and len(P.STAGES) == 3
    assert P.FILL not in P.STAGES and P.FILL.run is None and P.FILL.info == "last_mesh_fill"
    assert P.FILL.keywords == R.mesh_fill.FILL_KEYWORDS
    v, t = (torch.from_numpy(x) for x in M.tetrahedron())
    assert P.run_fill(None, v, t, None) == (v, t)


NAMES = ("rnb_mesh_fill_workspace_bytes", "rnb_mesh_loops_count", "rnb_mesh_loops_emit", "rnb_mesh_loops_mean",
         "rnb_mesh_fill_emit")


def test_the_bindings_cover_the_new_symbols_and_the_header_declares_them():
    N = R.native
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(R.__file__))), "include", "rnbneus.h")).read()
    lib = N.load()
    for name in NAMES:
        assert name in N.EXPORTED_SYMBOLS and N.signature(name)[0] is C.c_int
        assert f"int {name}(" in header and hasattr(lib, name)
    assert len(set(N.EXPORTED_SYMBOLS)) == len(N.EXPORTED_SYMBOLS)
    assert N.ABI_VERSION == 5 and lib.rnb_abi_version() == 5
    with pytest.raises(KeyError):
        N.signature("rnb_no_such_symbol")
    assert "mesh_fill.hip" in R.buildid.HIP_SOURCES if hasattr(R, "buildid") else True
    assert "boundary_loops" in R.__all__ and "fill_holes" in R.__all__


def _ws(V, T):
    out = C.c_int64(-7)
    return R.native.load().rnb_mesh_fill_workspace_bytes(V, T, C.byref(out)), out.value


def test_the_workspace_query():
    sizes = [0, 1, 1024, 1025, 10 ** 6, 2 ** 30]
    b = np.array([[_ws(V, T) for T in sizes] for V in sizes])
    assert (b[:, :, 0] == 0).all() and (b[:, :, 1] > 0).all() and (np.diff(b[:, :, 1], axis=0) > 0).all()
    for V, T in ((-1, 0), (0, -1), (2 ** 31, 0), (0, 1431655765)):
        assert _ws(V, T) == (-1, -7), (V, T)
    assert R.native.load().rnb_mesh_fill_workspace_bytes(1, 1, None) == -4
    N, a = R.native, (1000, 2000)
    need = _ws(*a)[1]
    assert N.workspace_bytes("mesh_fill", *a) == need and N.workspace("mesh_fill", "cpu", *a).numel() == need
    assert N.workspace("mesh_fill", "cpu", *a, floor=need + 17).numel() == need + 17


def test_the_library_checks_its_arguments_before_any_launch():
    """the pointers are made up: a call that got as far as a launch would need a device"""
    lib = R.native.load()
    p, big = C.c_void_p(4096), 1 << 40

    def count(T=4, V=8, tws=p, twsb=big, bl=p, bd=p, ws=p, wsb=big, counts=p):
        return lib.rnb_mesh_loops_count(T, V, tws, twsb, bl, bd, -1, ws, wsb, counts, None)

    def emit(T=4, V=8, bl=p, ws=p, wsb=big, L=2, B=6, longest=3, M_=0, off=p, lv=p, st=p, ed=p):
        return lib.rnb_mesh_loops_emit(T, V, bl, ws, wsb, L, B, longest, M_, off, lv, st, ed, None)

    def mean(vals=p, kind=0, V=8, C_=3, off=p, lv=p, L=2, B=6, ws=p, wsb=big, out=p):
        return lib.rnb_mesh_loops_mean(vals, kind, V, C_, off, lv, L, B, ws, wsb, out, None)

    def fill(v=p, V=8, t=p, T=4, off=p, lv=p, st=p, cen=p, L=2, B=6, ws=p, wsb=big, F_=1, N_=3, vo=p, to=p, fl=p):
        return lib.rnb_mesh_fill_emit(v, V, t, T, off, lv, st, cen, L, B, -1, ws, wsb, F_, N_, vo, to, fl, None)

    exact = _ws(8, 4)[1]
    for call in (count, emit, mean, fill):
        assert call(V=-1) == -1 and call(V=2 ** 31) == -1
        assert call(ws=None) == -4 and b"workspace" in lib.rnb_last_error_string()
        assert call(wsb=8) == -2 and call(wsb=exact - 1) == -2
    for call in (count, emit, fill):
        assert call(T=-1) == -1 and call(T=2 ** 31 - 1) == -1 and b"half-edges" in lib.rnb_last_error_string()
    assert count(tws=None) == -4 and count(twsb=8) == -2 and count(counts=None) == -4 and count(bl=None) == -4 and count(bd=None) == -4
    for call in (emit, mean, fill):
        assert call(L=-1) == -1 and call(L=9) == -1 and call(B=-1) == -1 and call(B=9) == -1
        assert call(off=None) == -4 and call(lv=None) == -4
    assert emit(longest=7) == -1 and emit(M_=7) == -1 and emit(st=None) == -4 and emit(ed=None) == -4 and emit(bl=None) == -4
    assert mean(kind=2) == -1 and mean(C_=-1) == -1 and mean(vals=None) == -4 and mean(out=None) == -4
    assert fill(F_=3) == -1 and fill(N_=7) == -1 and fill(F_=-1) == -1
    assert fill(v=None) == -4 and fill(t=None) == -4 and fill(vo=None) == -4 and fill(to=None) == -4
    assert fill(st=None) == -4 and fill(cen=None) == -4 and fill(fl=None) == -4
    assert fill(V=2 ** 31 - 1, L=1, B=1, F_=1, N_=1, wsb=1 << 50) == -1 and b"2^31 - 1" in lib.rnb_last_error_string()


def test_the_ngon_area_and_the_mean_bound():
    assert F.ngon_area(4) == pytest.approx(2.0) and F.ngon_area(10 ** 6) == pytest.approx(math.pi, rel=1e-10)
    x = np.array([[1.0, -2.0], [3.0, 2.0]])
    assert F.mean_bound(x, np.array([0, 1])).tolist() == [2 * 2.0 ** -52 * 2.0, 2 * 2.0 ** -52 * 2.0]
    assert F.mean_rows(x, np.array([0, 1])).tolist() == [2.0, 0.0]
    assert np.isnan(F.mean_rows(np.array([[np.inf], [1.0]]), np.array([0, 1]))[0])
