"""The mesh topology audit on the device (rnb_neus_fork_amd.mesh_topology, csrc/mesh_topology.hip) against the numpy reference
of tests/mesh_topology_ref.py.  For every case: counts, flags, edges, edge_use, edge_triangle, boundary labels and degrees and
the per-component integer table with array_equal; two runs bit-equal in everything, the volume included; the volume per
component within n_c 2^-55 M_c + 2^-52 |ref| of the reference's fsum (M_c the component's largest |term|: every term is
rounded to the unit 2^(e_c - 54); two final roundings, the device's conversion and fsum's), NaN in the same places.  The
shapes are the smallest at which each mechanism can go wrong (the issue lists them); every case prints one TOPOLOGY line."""
import time

import numpy as np
import pytest
import torch

from tests import mesh_topology_ref as M
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device
from tests.mc_shapes import sphere

pytestmark = pytest.mark.gpu

_REF = {}
COUNT_KEYS = ("n_edges", "n_boundary", "n_manifold", "n_flipped", "n_nonmanifold", "n_degenerate", "n_invalid",
              "n_boundary_components")


def _np(x):
    return x.detach().cpu().numpy()


def _run(R, v, t, n_vertices=None, **kw):
    tt = torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32)).to(device())
    vv = None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(device())
    return R.mesh_topology(tt, n_vertices if v is None else None, vv, **kw)


def _arrays(out):
    """the report as the reference lays it out"""
    a = {"counts": np.array([out[k] for k in COUNT_KEYS], dtype=np.int64)}
    a.update({k: _np(out[k]) for k in ("triangle_flags", "vertex_flags", "boundary_labels", "boundary_degree", "edges",
                                       "edge_use", "edge_triangle")})
    c = out["components"]
    a["table"] = np.concatenate([_np(c["edges"]), *[_np(c[k])[:, None] for k in ("triangles", "degenerate", "holes", "vertices")]],
                                axis=1)
    a.update(labels=_np(c["labels"]), euler=_np(c["euler"]), closed=_np(c["closed"]), genus=_np(c["genus"]))
    a["n_components"], a["boundary_simple"] = c["n_components"], out["boundary_simple"]
    if "volume" in c:
        a["volume"] = _np(c["volume"])
    return a


def _check(R, tag, v, t, ref=None):
    """the device report twice, against the reference; returns (arrays, reference)"""
    t0 = time.perf_counter()
    if ref is None:
        if tag not in _REF:
            _REF[tag] = M.topology(t, len(v), v)
        ref = _REF[tag]
    out = _run(R, v, t, edges=True)
    got, again = _arrays(out), _arrays(_run(R, v, t, edges=True))
    diff = M.equal(got, {**ref, "volume": got["volume"]})      # (the volume has its own bound below)
    assert diff is None, f"{tag}: {diff} differs from the reference"
    for k in M.INT_KEYS:
        assert got[k].dtype == ref[k].dtype, (tag, k, got[k].dtype, ref[k].dtype)
        assert np.array_equal(got[k], again[k]), f"{tag}: {k} differs between two runs"
    assert got["volume"].tobytes() == again["volume"].tobytes(), f"{tag}: the volume differs between two runs"
    nan = np.isnan(ref["volume"])
    assert np.array_equal(np.isnan(got["volume"]), nan), f"{tag}: NaN volumes in other places"
    err = np.abs(got["volume"] - ref["volume"])[~nan]
    bound = ref["volume_bound"][~nan]
    worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"TOPOLOGY {tag}: V {len(v)} T {len(t)} counts {got['counts'].tolist()} C {got['n_components']}; volumes "
          f"{got['volume'][:3].tolist()}, error at most {worst:.2e} of its bound; {time.perf_counter() - t0:.2f} s")
    assert (err <= bound).all(), f"{tag}: volume error {err.max():.3e} above the bound (ratio {worst:.2e})"
    assert R.watertight(out) == bool(ref["closed"].all() and ref["counts"][6] == 0)
    return got, ref


@pytest.mark.parametrize("name", list(M.small_shapes()))
def test_small_closed_forms(R, name):
    v, t = M.small_shapes()[name]
    got, _ = _check(R, name, v, t)
    if name == "tetrahedron":
        assert got["counts"].tolist() == [6, 0, 6, 0, 0, 0, 0, 0] and got["euler"][0] == 2 and got["closed"][0]
    if name == "one reversed":
        assert got["counts"][3] == 3
    if name == "bow tie":
        assert got["boundary_degree"].max() == 4 and not got["boundary_simple"]
    if name == "all interleaved":
        assert got["n_components"] == 7 and got["counts"][7] == 3


def test_degenerate_input(R):
    v, t = M.degenerate_input()
    got, _ = _check(R, "degenerate input", v, t)
    assert got["counts"][5] == 1 and got["counts"][6] == 2 and (got["counts"][3] > 0 or got["counts"][4] > 0)
    assert (got["vertex_flags"][10:] == 8).all() and (got["vertex_flags"][:10] & 8 == 0).all()
    assert sorted(got["triangle_flags"][10:13].tolist()) == [8, 16, 16]
    v = v.copy()
    v[9, 1] = np.nan                                           # reaches the proper triangle (0, 9, 8): that component's volume
    got, _ = _check(R, "degenerate input with a NaN corner", v, t)
    assert np.isnan(got["volume"]).sum() == 1


def test_empty_meshes(R):
    none = np.zeros((0, 3), dtype=np.int32)
    got, _ = _check(R, "T = 0", np.zeros((5, 3)), none)
    assert got["counts"].tolist() == [0] * 8 and (got["vertex_flags"] == 8).all() and (got["boundary_labels"] == -1).all()
    got, _ = _check(R, "V = 0", np.zeros((0, 3)), np.array([[0, 1, 2], [0, 0, 0]], dtype=np.int32))
    assert got["counts"].tolist() == [0, 0, 0, 0, 0, 0, 2, 0] and got["triangle_flags"].tolist() == [16, 16]
    got, _ = _check(R, "V = 0, T = 0", np.zeros((0, 3)), none)
    assert got["counts"].tolist() == [0] * 8 and got["n_components"] == 0


@pytest.mark.parametrize("mixed", [False, True])
def test_one_hot_slot(R, mixed):
    """1,000 half-edges of one key contend for one table slot and one counter"""
    v, t = M.fan(1000, mixed)
    got, _ = _check(R, f"fan mixed={mixed}", v, t)
    assert got["edge_use"][0].tolist() == ([666, 334] if mixed else [1000, 0]) and got["edges"][0].tolist() == [0, 1]


@pytest.mark.parametrize("n", [85, 86, 255, 256, 257, 341, 342, 1023, 1024, 1025])
def test_block_and_tile_edges(R, n):
    """3T one below, at and above 256 and 1024, and T and V likewise"""
    v, t = M.strip(n)
    got, _ = _check(R, f"strip {n}", v, t)
    assert got["counts"][0] == 2 * n + 1 and got["counts"][1] == n + 2 and got["counts"][7] == 1 and got["boundary_simple"]


def test_past_the_second_scan_level_closed(R):
    v, t = M.torus_grid(600, 300)
    assert 3 * len(t) > 2 ** 20 and 3 * len(t) // 2 > 2 ** 19
    got, _ = _check(R, "torus 600x300", v, t)
    assert got["counts"].tolist() == [540000, 0, 540000, 0, 0, 0, 0, 0] and got["euler"].tolist() == [0] and got["genus"].tolist() == [1]


def test_past_the_second_scan_level_with_holes(R):
    v, t = M.torus_with_holes()
    got, ref = _check(R, "torus 600x300 holes", v, t)
    assert 100 <= ref["counts"][7] <= 1000, "checked on the CPU with the reference alone: neither trivial case"
    assert got["table"][0, 6] == ref["counts"][7]


def _mc(R, c, r, n=48):
    v, t = R.marching_cubes(torch.from_numpy(sphere(n, r, c)).to(device()), 0.0)
    return v, t


def test_marching_cubes_sphere_inside_the_box(R):
    v, t = _mc(R, (0.05, -0.02, 0.03), 0.6)
    got, _ = _check(R, "mc sphere", _np(v), _np(t))
    assert got["closed"].tolist() == [True] and got["euler"].tolist() == [2] and 2 * got["counts"][0] == 3 * len(_np(t))


def test_the_pipeline_chain_on_a_sphere_cut_by_the_box_wall(R):
    """what the feature exists for: the cut sphere, then after simplify_mesh at 3 voxels, compact_triangles with a seeded
    keep, and clean_mesh — the full report against the reference each time"""
    v, t = _mc(R, (0.7, 0.0, 0.0), 0.6)
    got, _ = _check(R, "mc cut sphere", _np(v), _np(t))
    assert got["counts"][7] == 1 and got["boundary_simple"] and got["table"][0, 6] == 1 and got["genus"].tolist() == [0]
    s = R.simplify_mesh(v, t, cell_size=3.0)
    got, _ = _check(R, "cut sphere simplified", _np(s["vertices"]), _np(s["triangles"]))
    assert got["counts"][5] == 0
    keep = torch.from_numpy(np.random.default_rng(9).random(s["triangles"].shape[0]) < 0.8).to(device())
    c = R.compact_triangles(s["vertices"], s["triangles"], keep)
    got, _ = _check(R, "cut sphere compacted", _np(c["vertices"]), _np(c["triangles"]))
    assert got["counts"][1] > 30, "the seeded keep opens boundaries"
    k = R.clean_mesh(c["vertices"], c["triangles"], keep_largest=1)
    got, _ = _check(R, "cut sphere cleaned", _np(k["vertices"]), _np(k["triangles"]))
    assert got["n_components"] == 1


def test_attributes_of_the_python_layer(R):
    v, t = M.small_shapes()["all interleaved"]
    full = _run(R, v, t, edges=True)
    plain = _run(R, v, t)
    assert not {"edges", "edge_use", "edge_triangle"} & set(plain) and {"edges", "edge_use", "edge_triangle"} <= set(full)
    nob = _run(R, v, t, boundary=False)
    assert not {"boundary_labels", "boundary_degree", "n_boundary_components", "boundary_simple"} & set(nob)
    assert (_np(nob["components"]["holes"]) == -1).all() and (_np(nob["components"]["genus"]) == -1).all()
    assert torch.equal(nob["components"]["euler"], full["components"]["euler"])
    noc = _run(R, v, t, components=False)
    assert "components" not in noc and noc["n_boundary_components"] == full["n_boundary_components"]
    none = _run(R, None, t, n_vertices=len(v), components=False, boundary=False)
    assert torch.equal(none["triangle_flags"], full["triangle_flags"]) and torch.equal(none["vertex_flags"], full["vertex_flags"])
    assert "volume" not in _run(R, None, t, n_vertices=len(v))["components"]
    # the ABI level: NULL boundary arrays make no union-find launch and counts[7] = -1
    lib, dev = R.native.load(), device()
    tt = torch.from_numpy(t).to(dev)
    ws = R.native.workspace("mesh_topology", dev, len(v), len(t))
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    tf, vf = torch.empty(len(t), dtype=torch.uint8, device=dev), torch.empty(len(v), dtype=torch.uint8, device=dev)
    with R.native.on_device(dev) as stream:
        R.native.check(lib.rnb_mesh_topology_count(R.native.ptr(tt), len(t), len(v), R.native.ptr(ws), ws.numel(),
                                                   R.native.ptr(counts), R.native.ptr(tf), R.native.ptr(vf), None, None, stream))
    assert counts.cpu().tolist() == [full[k] for k in COUNT_KEYS[:7]] + [-1]
    assert torch.equal(tf, full["triangle_flags"])
