"""Host side of the mesh ray casting (rnb_mesh_raycast of include/rnbneus.h, rnb_neus_fork_amd.mesh_raycast): the numpy
reference the GPU tests compare against (tests/mesh_raycast_ref.py) agrees with its second formulation and closes a
closed surface, the symbol is declared, bound and exported, every argument check comes before anything touches a device,
and the parts that are torch only (interpolation, the angular error) do what they say.  No GPU."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import rnb_neus_fork_amd as R
from rnb_neus_fork_amd import mesh_raycast as M
from tests import mesh_raycast_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_INVALID, E_NULL = 0, -1, -4


def test_symbol_is_declared_bound_and_exported():
    lib = R.native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnbneus.h")).read(), flags=re.S)
    name = "rnb_mesh_raycast"
    assert name in R.native.EXPORTED_SYMBOLS and hasattr(lib, name)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/rnbneus.h"
    restype, argtypes = R.native._SIGNATURES[name]
    decls = [d.strip() for d in m.group(1).split(",")]
    assert restype is C.c_int and len(argtypes) == len(decls) == 16
    for decl, ct in zip(decls, argtypes):
        if "rnb_mesh_bins*" in decl:
            assert ct is C.POINTER(R.native.MeshBins), decl
        elif "*" in decl or decl.startswith("rnb_stream_t"):
            assert ct is C.c_void_p, decl
        else:
            assert ct is {"int64_t": C.c_int64, "int32_t": C.c_int32}[decl.split()[0]], decl
    assert lib.rnb_abi_version() == 5 and R.native.ABI_VERSION == 5
    from rnb_neus_fork_amd import buildid
    assert "mesh_raycast.hip" in buildid.HIP_SOURCES and buildid.EXTRA_FLAGS["mesh_raycast.hip"] == ["-ffp-contract=off"]
    assert {"mesh_view_maps", "normal_angular_error"} <= set(R.__all__)
    assert all(hasattr(R.MeshIndex, n) for n in ("raycast", "interpolate", "visible"))


def _bins(dims=(4, 4, 4), cell=0.5, origin=(0.0, 0.0, 0.0)):
    return R.native.MeshBins((C.c_double * 3)(*origin), cell, (C.c_int32 * 3)(*dims), 0)


def test_argument_checks_come_before_any_launch():
    """Every call below returns before a stream or the device is touched: the pointers are made up, and a call that got
    as far as a launch would need a device."""
    lib = R.native.load()
    p = C.c_void_p(4096)           # never dereferenced on the host
    good, COVER = _bins(), R.native.MESH_BINS_COVER
    bad_bins = [_bins(dims=(0, 4, 4)), _bins(dims=(4, -1, 4)), _bins(dims=(512, 512, 512)), _bins(cell=0.0), _bins(cell=-1.0),
                _bins(cell=float("nan")), _bins(cell=float("inf")), _bins(origin=(0.0, float("nan"), 0.0)),
                _bins(origin=(float("inf"), 0.0, 0.0)), _bins(origin=(1e308, 0.0, 0.0), cell=1e307, dims=(64, 1, 1))]

    def cast(o=p, d=p, lo=p, hi=p, N=5, bins=good, cs=p, entries=p, E=9, corners=p, T=4, flags=COVER, t=p, tr=p, bary=p):
        return lib.rnb_mesh_raycast(o, d, lo, hi, N, C.byref(bins) if bins is not None else None, cs, entries, E, corners, T,
                                    flags, t, tr, bary, None)

    assert cast(flags=0) == E_INVALID and b"RNB_MESH_BINS_COVER" in lib.rnb_last_error_string(), "a grid that may not cover the mesh"
    assert cast(flags=2) == E_INVALID and cast(flags=3) == E_INVALID and cast(flags=-1) == E_INVALID
    assert b"flag" in lib.rnb_last_error_string()
    assert cast(N=-1) == E_INVALID and cast(N=2 ** 31) == E_INVALID
    assert cast(E=-1) == E_INVALID and cast(E=2 ** 31) == E_INVALID and cast(T=-1) == E_INVALID and cast(T=2 ** 31) == E_INVALID
    assert all(cast(bins=b) == E_INVALID for b in bad_bins)
    assert cast(bins=None) == E_NULL and cast(o=None) == E_NULL and cast(d=None) == E_NULL
    assert cast(cs=None) == E_NULL and cast(entries=None) == E_NULL and cast(corners=None) == E_NULL
    assert cast(t=None, tr=None, bary=None) == E_NULL and b"output" in lib.rnb_last_error_string()
    assert cast(N=0, o=None, d=None) == OK                                               # no ray: nothing launched
    assert cast(N=0, flags=0) == E_INVALID and cast(N=0, bins=bad_bins[0]) == E_INVALID  # still refused


class _FakeIndex:
    """what the Python checks read of a MeshIndex before they reach the library"""
    def __init__(self, covers=True, device=torch.device("cpu")):
        self.covers, self.device = covers, device


def test_python_argument_checks_fire_on_the_host():
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64)
    o, d = torch.zeros(4, 3, dtype=torch.float64), torch.ones(4, 3, dtype=torch.float64)
    idx = _FakeIndex()
    for bad in (o[:, :2], o.reshape(-1), o.numpy(), o.to(torch.int64), o.to(torch.float16)):
        with pytest.raises(ValueError, match="origins"):
            M.raycast(idx, bad, d)
        with pytest.raises(ValueError, match="directions"):
            M.raycast(idx, o, bad)
        with pytest.raises(ValueError, match="points"):
            M.visible(idx, bad, v[0])
    with pytest.raises(ValueError, match="differ in shape"):
        M.raycast(idx, o, d[:3])
    with pytest.raises(ValueError, match="without grid="):
        M.raycast(_FakeIndex(covers=False), o, d)
    for eye in (v[0, :2], v[:2], [0.0, 0.0, 0.0], v[0].to(torch.int64)):
        with pytest.raises(ValueError, match="eye"):
            M.visible(idx, o, eye)
    for tol in (-0.1, 1.0, float("nan"), "x", True):
        with pytest.raises(ValueError, match="rel_tol"):
            M.visible(idx, o, v[0], rel_tol=tol)
    # valid arguments on CPU tensors: there is no CPU path (float32 rays are valid arguments)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        M.raycast(idx, o, d)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        M.raycast(idx, o.float(), d.float(), 0.0, 1.0)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        M.visible(idx, o, v[0])
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        R.mesh_view_maps(idx, o, d)
    with pytest.raises(ValueError, match="shape"):
        R.mesh_view_maps(idx, o, d, shape=(3, 2))
    with pytest.raises(ValueError, match="not both"):
        R.mesh_view_maps(idx, {"rays_o": o, "rays_d": d, "H": 2, "W": 2}, d)
    for bad_o, bad_d, match in ((o.numpy(), d, "rays_o"), (o, [1.0, 0.0, 0.0], "rays_d"), (o, d[:, :2], "rays_d"), (o, None, "rays_d"),
                                ({"rays_o": o}, None, "rays_o and rays_d"), ({"rays_o": o, "rays_d": "x"}, None, "rays_d")):
        with pytest.raises(ValueError, match=match):
            R.mesh_view_maps(idx, bad_o, bad_d)
    for shape in (4, (2.0, 2), (2, 2, 1), "22"):
        with pytest.raises(ValueError, match="shape"):
            R.mesh_view_maps(idx, o, d, shape=shape)
    # a bound is a number, a one-element tensor or one value per ray, and nothing else
    for bad in (torch.zeros(3), torch.zeros(4, 2), torch.zeros(2, 2), torch.zeros(4, dtype=torch.int64), "0", True):
        with pytest.raises(ValueError, match="t_min"):
            M.raycast(idx, o, d, t_min=bad)
    with pytest.raises(RuntimeError, match="GPU tensors only"):                          # a valid bound gets as far as the device
        M.raycast(idx, o[:1], d[:1], t_min=torch.zeros(()))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        R.mesh_view_maps(idx, {"rays_o": o.float(), "rays_d": d.float(), "H": 2, "W": 2})


def test_reference_against_its_second_formulation():
    """rays aimed well inside triangles: both formulations hit the same triangle at the same t up to rounding"""
    case = F.torus_rays()
    v, t = case["vertices"], case["triangles"]
    rng = np.random.default_rng(3)
    w = rng.uniform(0.1, 1.0, (len(t), 3))
    w /= w.sum(axis=1, keepdims=True)                         # every weight >= 0.1 / 2.1: clear of the edges
    tgt = (v[t] * w[:, :, None]).sum(axis=1)
    o = rng.normal(size=(len(t), 3))
    o = 3.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = tgt - o
    t1, tr1, b1 = F.raycast_all(o, d, v, t)
    t2, tr2, _ = F.raycast_all(o, d, v, t, fn="mt")
    assert (tr1 >= 0).all() and (t1 <= 1.0 + 1e-12).all(), "every ray meets the mesh at its target or before"
    # t is a ratio whose denominator is proportional to the cosine between ray and face normal: an error of a few
    # 2^-52 L (L = 4 bounds every coordinate and |d|) in the numerator is 1 / cos as much in t.  64 leaves room for two
    # evaluation orders.
    cos = np.abs((F.face_normals(v, t)[tr1] * d).sum(axis=1)) / np.linalg.norm(d, axis=1)
    tol = 64 * F.EPS * 4.0 / cos
    at_target = np.abs(t1 - 1.0) <= tol
    assert at_target.mean() > 0.2 and (tr1[at_target] == np.flatnonzero(at_target)).all()
    assert np.abs(b1[at_target] - w[at_target]).max() < 1e-9, "bary = the weights of (A, B, C)"
    clear = b1.min(axis=1) > 1e-6
    assert clear.mean() > 0.99
    assert (tr1[clear] == tr2[clear]).all() and (np.abs(t1 - t2)[clear] <= tol[clear]).all()
    # the hit point lies on the hit triangle and on the ray
    pt = (v[t[tr1]] * b1[:, :, None]).sum(axis=1)
    assert (np.abs(pt - (o + t1[:, None] * d)).max(axis=1) <= 4.0 * tol).all()
    # documented specials
    tn, trn, bn = F.raycast_all([[0, 0, 0], [np.nan, 0, 0], [0, 0, 0], [0, 0, 0], [5, 5, 5]],
                                [[0, 0, 0], [1, 0, 0], [np.inf, 0, 0], [1, 0, 0], [1, 0, 0]], v, t, [0, 0, 0, np.nan, 0])
    assert np.isnan(tn[:4]).all() and np.isposinf(tn[4]) and (trn == -1).all() and np.isnan(bn).all()
    # the torus case itself: every group does what its name says
    ref_t, ref_tr, _ = case["ref"]
    assert len(ref_t) == 2000 and not np.isnan(ref_t).any()
    assert (ref_tr[:500] >= 0).all(), "from inside a closed surface every ray meets it"
    assert (ref_tr[500:1000] >= 0).mean() > 0.9 and (ref_tr[1000:1300] == -1).all() and (ref_tr[1300:1600] == -1).all()
    assert (ref_tr[1600:1700] >= 0).all() and np.array_equal(ref_t[1600:1700], case["t_max"][1600:1700]), "t_max is inclusive"
    assert (ref_tr[1700:] >= 0).mean() > 0.5 and (ref_t[1700:][ref_tr[1700:] >= 0] >= 0).all()


def test_the_watertight_test_closes_a_closed_surface_and_moeller_trumbore_does_not():
    case = F.watertight_case()
    v, t, o, d = case["vertices"], case["triangles"], case["origins"], case["directions"]
    assert len(o) == 3 * 2562
    ref_t, ref_tr, ref_b = case["ref"]
    assert (ref_tr >= 0).all(), f"the watertight test misses {(ref_tr < 0).sum()} rays of a closed surface"
    assert np.abs(ref_t - 1.0).max() < 1e-12 and ref_b.min() >= 0.0
    mt = F.raycast_all(o, d, v, t, fn="mt")[1].reshape(3, -1)
    missed = (mt < 0).sum(axis=1)
    print(f"Moeller-Trumbore misses {missed.tolist()} of 2562 rays per origin; the watertight test none")
    assert (missed > 0).all(), "rays through vertices and edges: Moeller-Trumbore leaves pinholes"
    # an exact tie goes to the smaller index: the same triangle twice, and a ray in the plane x = 0 through an edge in it
    t1, tr1, _ = F.raycast_all(o[:500], d[:500], v, np.concatenate([t, t]))
    assert np.array_equal(t1, ref_t[:500]) and np.array_equal(tr1, ref_tr[:500])
    sq = np.array([[0.0, -1.0, 1.0], [0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [-1.0, 0.0, 1.0]])
    tt, tri, bb = F.raycast_all([[0.0, 0.25, 0.0]], [[0.0, 0.0, 2.0]], sq, [[1, 0, 3], [0, 1, 2]])
    assert tt[0] == 0.5 and tri[0] == 0 and bb[0].tolist() == [0.625, 0.375, 0.0], "zero counts as inside, on both sides"


def test_interpolate_on_hand_made_hits():
    tri = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    index = types.SimpleNamespace(triangles=tri, n_vertices=4)
    hits = {"triangle": torch.tensor([0, 1, -1, 1], dtype=torch.int32),
            "bary": torch.tensor([[0.5, 0.25, 0.25], [0.0, 0.0, 1.0], [float("nan")] * 3, [0.25, 0.5, 0.25]], dtype=torch.float64)}
    vals = torch.tensor([[1.0, 10.0], [2.0, 20.0], [4.0, 40.0], [8.0, 80.0]], dtype=torch.float64)
    out = M.interpolate(index, hits, vals)
    assert out.shape == (4, 2) and out.dtype == torch.float64
    assert out[0].tolist() == [2.0, 20.0] and out[1].tolist() == [8.0, 80.0] and out[3].tolist() == [4.0, 40.0]
    assert torch.isnan(out[2]).all()
    flat = M.interpolate(index, hits, vals[:, 0].float())
    assert flat.shape == (4,) and flat.dtype == torch.float32 and flat[0] == 2.0 and torch.isnan(flat[2])
    assert M.interpolate(index, hits, torch.arange(4)).tolist()[:2] == [0.75, 3.0]
    for bad in (vals[:3], vals.reshape(-1, 1, 2), vals.numpy()):
        with pytest.raises(ValueError, match="vertex_values"):
            M.interpolate(index, hits, bad)
    with pytest.raises(ValueError, match="hits"):
        M.interpolate(index, {"triangle": hits["triangle"]}, vals)
    with pytest.raises(ValueError, match="hits"):
        M.interpolate(index, {"triangle": hits["triangle"], "bary": hits["bary"][:3]}, vals)


def test_the_statistics_never_read_a_value_on_the_host():
    """On meta tensors there is no data: any `.item()`, `bool()` of a tensor or index by a 0-dim tensor — each a hidden
    host synchronisation on a GPU — raises.  `angular_error_statistics` and `interpolate` must run through, which leaves
    `normal_angular_error` with the one synchronisation it states: the read of the [4] tensor."""
    n = torch.empty(6, 5, 3, dtype=torch.float64, device="meta")
    stats = M.angular_error_statistics(n, n, torch.empty(6, 5, dtype=torch.bool, device="meta"))
    assert stats.shape == (4,) and stats.dtype == torch.float64 and stats.device.type == "meta"
    assert M.angular_error_statistics(n.float(), n.float()).shape == (4,)
    index = types.SimpleNamespace(triangles=torch.empty(7, 3, dtype=torch.int32, device="meta"), n_vertices=9)
    hits = {"triangle": torch.empty(11, dtype=torch.int32, device="meta"), "bary": torch.empty(11, 3, dtype=torch.float64, device="meta")}
    out = M.interpolate(index, hits, torch.empty(9, 3, dtype=torch.float32, device="meta"))
    assert out.shape == (11, 3) and out.device.type == "meta"


def test_normal_angular_error_on_hand_made_maps():
    rng = np.random.default_rng(11)
    n = rng.normal(size=(6, 5, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    a = torch.from_numpy(n)
    same = R.normal_angular_error(a, a)
    assert same == {"mean": 0.0, "median": 0.0, "rms": 0.0, "count": 30}
    # every normal rotated by 7.5 degrees about an axis perpendicular to it
    axis = np.cross(n, rng.normal(size=3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    ang = math.radians(7.5)
    rot = torch.from_numpy(n * math.cos(ang) + np.cross(axis, n) * math.sin(ang))
    e = R.normal_angular_error(a, rot)
    assert e["count"] == 30 and all(abs(e[k] - 7.5) < 1e-9 for k in ("mean", "median", "rms"))
    # known angles, a mask, and pixels that do not count: NaN, zero normals
    b = a.clone().reshape(-1, 3)
    angles = [0.0, 10.0, 20.0, 90.0, 180.0]
    for k, deg in enumerate(angles):
        r = math.radians(deg)
        b[k] = torch.from_numpy(n.reshape(-1, 3)[k] * math.cos(r) + np.cross(axis.reshape(-1, 3)[k], n.reshape(-1, 3)[k]) * math.sin(r))
    b[5] = float("nan")
    b[6] = 0.0
    mask = torch.zeros(30, dtype=torch.bool)
    mask[:8] = True
    e = R.normal_angular_error(a, b.reshape(6, 5, 3) * 3.0, mask.reshape(6, 5))        # 0 10 20 90 180 | nan zero | 0: 6 count
    assert e["count"] == 6
    assert abs(e["mean"] - 50.0) < 1e-9 and abs(e["median"] - 15.0) < 1e-9
    assert abs(e["rms"] - math.sqrt(sum(x * x for x in angles) / 6.0)) < 1e-9
    none = R.normal_angular_error(a, a, torch.zeros(6, 5))
    assert none["count"] == 0 and all(math.isnan(none[k]) for k in ("mean", "median", "rms"))
    assert R.normal_angular_error(a.float(), rot.float())["count"] == 30
    # one pixel, and an odd count: the median is the middle angle
    one = R.normal_angular_error(a[:1, :1], rot[:1, :1])
    assert one["count"] == 1 and abs(one["median"] - 7.5) < 1e-9
    mask3 = torch.zeros(30, dtype=torch.bool)
    mask3[1:4] = True
    assert abs(R.normal_angular_error(a, b.reshape(6, 5, 3), mask3.reshape(6, 5))["median"] - 20.0) < 1e-9
    with pytest.raises(ValueError, match="one shape"):
        R.normal_angular_error(a, a[:5])
    with pytest.raises(ValueError, match="mask"):
        R.normal_angular_error(a, a, torch.ones(7))
