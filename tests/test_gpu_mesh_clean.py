"""Mesh cleanup on the device (csrc/mesh_clean.hip through `mesh_components`, `clean_mesh` and the renderer's `clean=`)
against the numpy reference of tests/mesh_components_ref.py.

Labels, counts, bounding boxes, vertices and triangles are integers or copies with a canonical definition: every such
comparison is `array_equal`.  The area alone is a floating-point sum: per component
    |got - ref| <= (n_c + 16) 2^-52 S_c,   S_c = sum of 0.5 |e1| |e2| over the component's n_c triangles
(n_c 2^-52 S_c: two summation orders; 16 x 2^-52 S_c: a few ulps of evaluation order per triangle), and two runs are
bit-equal.  References are computed once per mesh and shared; callers must not modify what they get."""
import numpy as np
import pytest
import torch

from oracle import mc_oracle as M
from oracle import rnb_oracle as O
from tests import mesh_attrs_util as U
from tests import mesh_components_ref as F
from tests import parity as P
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device

pytestmark = pytest.mark.gpu

LO, HI = U.LO, U.HI
_REF = {}


def _ref(key, make):
    """(vertices, triangles, labels, C, stats, area bound) of a named mesh, once"""
    if key not in _REF:
        v, t = make()
        v, t = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3)
        labels, n = F.components(t, len(v))
        _REF[key] = (v, t, labels, n, F.stats(t, labels, n, v), F.area_bound(v, t, labels, n))
    return _REF[key]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device())


def _np(x):
    return x.cpu().numpy()


def _check_components(R, key, make, with_coords=True):
    v, t, labels, n, st, bound = _ref(key, make)
    got = R.mesh_components(_dev(t), vertices=_dev(v)) if with_coords else R.mesh_components(_dev(t), n_vertices=len(v))
    assert got["n_components"] == n and got["labels"].dtype == torch.int32
    assert np.array_equal(_np(got["labels"]), labels), f"{key}: labels"
    assert np.array_equal(_np(got["triangles"]), st["triangles"]) and got["triangles"].dtype == torch.int64
    assert np.array_equal(_np(got["vertices"]), st["vertices"]) and got["vertices"].dtype == torch.int64
    if not with_coords:
        assert set(got) == {"labels", "n_components", "triangles", "vertices"}
        return got
    assert np.array_equal(_np(got["bbox_min"]), st["bbox_min"], equal_nan=True), f"{key}: bbox_min"
    assert np.array_equal(_np(got["bbox_max"]), st["bbox_max"], equal_nan=True), f"{key}: bbox_max"
    area = _np(got["area"])
    assert np.array_equal(np.isnan(area), np.isnan(st["area"]))
    ok = ~np.isnan(area)
    err = np.abs(area - st["area"])[ok]
    worst = float((err / np.maximum(bound[ok], 1e-300)).max()) if ok.any() else 0.0
    print(f"{key}: C = {n}, area |dev - ref| at most {worst:.3f} of (n_c + 16) 2^-52 S_c")
    assert (err <= bound[ok]).all(), f"{key}: area off by {worst:.2f} of the bound"
    again = R.mesh_components(_dev(t), vertices=_dev(v))
    for k in ("labels", "triangles", "vertices", "area", "bbox_min", "bbox_max"):
        assert np.array_equal(_np(again[k]), _np(got[k]), equal_nan=True), f"{key}: {k} differs between two runs"
    return got


def _check_clean(R, key, make, **kw):
    v, t = _ref(key, make)[:2]
    attrs = {"id": _dev(np.arange(len(v), dtype=np.float32)), "pair": _dev(np.stack([v[:, 0], -v[:, 2]], axis=1))}
    got = R.clean_mesh(_dev(v), _dev(t), attributes=attrs, **kw)
    v1, t1, index, keep, st = F.clean(v, t, **kw)
    assert got["vertices"].dtype == torch.float64 and got["triangles"].dtype == torch.int32
    assert np.array_equal(_np(got["vertices"]), v1, equal_nan=True) and _np(got["vertices"]).shape == v1.shape, f"{key} {kw}"
    assert np.array_equal(_np(got["triangles"]), t1) and _np(got["triangles"]).shape == t1.shape, f"{key} {kw}"
    assert got["vertex_index"].dtype == torch.int64 and np.array_equal(_np(got["vertex_index"]), index)
    assert np.array_equal(_np(got["vertices"]), v[_np(got["vertex_index"])], equal_nan=True)
    assert np.array_equal(_np(got["attributes"]["id"]), index.astype(np.float32))
    assert np.array_equal(_np(got["attributes"]["pair"]), _np(attrs["pair"])[index], equal_nan=True)
    info = got["info"]
    assert info["n_components"] == len(keep) and np.array_equal(_np(info["kept"]), np.flatnonzero(keep))
    assert info["n_vertices"] == (len(v), len(v1)) and info["n_triangles"] == (len(t), len(t1))
    assert np.array_equal(_np(info["measure_kept"]), _np(info["measure"])[keep], equal_nan=True)
    return got, keep


# ---- volume A: a big sphere and two floaters whose vertices interleave -------------------------------------------------
def _mc_on_device(R, u):
    v, t = R.marching_cubes(_dev(u), 0.0)
    return _np(v), _np(t)


def test_volume_a_components_and_cleaning(R):
    make = lambda: _mc_on_device(R, F.volume_a())             # noqa: E731
    v, t, labels, n, st, _ = _ref("A", make)
    vo, to = M.marching_cubes(F.volume_a(), 0.0)
    assert np.array_equal(v, vo) and np.array_equal(t, to) and n == 3 and st["triangles"].tolist() == [2940, 560, 204]
    _check_components(R, "A", make)
    _check_components(R, "A", make, with_coords=False)
    # keep_largest=1 is the device marching cubes of the big sphere's volume alone, bit for bit
    got, keep = _check_clean(R, "A", make, keep_largest=1)
    vb, tb = _mc_on_device(R, F.volume_a(spheres=F.A_SPHERES[:1]))
    assert keep.tolist() == [True, False, False]
    assert np.array_equal(_np(got["vertices"]), vb) and np.array_equal(_np(got["triangles"]), tb)
    for kw, want in (({"keep_largest": 2}, [1, 1, 0]), ({"min_fraction": 0.1}, [1, 1, 0]), ({"min_fraction": 0.5}, [1, 0, 0]),
                     ({"min_triangles": 205}, [1, 1, 0]), ({"by": "triangles", "min_fraction": 0.1}, [1, 1, 0]),
                     ({"by": "triangles", "keep_largest": 3, "min_triangles": 561}, [1, 0, 0]),
                     ({"min_fraction": 1.0, "min_triangles": 10 ** 6}, [0, 0, 0])):
        assert _check_clean(R, "A", make, **kw)[1].tolist() == [bool(x) for x in want], kw
    # no criteria: a marching-cubes mesh comes back unchanged
    got, keep = _check_clean(R, "A", make)
    assert keep.all() and np.array_equal(_np(got["vertices"]), v) and np.array_equal(_np(got["triangles"]), t)


# ---- the noise volume: 370 components of many sizes, ties in triangle count ----------------------------------------------
def _noise_mesh(variant):
    v, t = M.marching_cubes(F.noise_volume(), 0.0)
    rng = np.random.default_rng(17)
    if variant == "vertices_permuted":
        return F.renumber(v, t, rng.permutation(len(v)))
    if variant == "triangles_permuted":
        return v, t[rng.permutation(len(t))]
    return v, t


@pytest.mark.parametrize("variant", ["as_emitted", "vertices_permuted", "triangles_permuted"])
def test_noise_volume_all_components_and_the_tie_rule(R, variant):
    key = "noise_" + variant
    make = lambda: _noise_mesh(variant)                       # noqa: E731
    v, t, labels, n, st, _ = _ref(key, make)
    assert n == 370 and len(np.unique(st["triangles"])) < n
    _check_components(R, key, make)
    if variant != "as_emitted":     # the labels changed by the id rule alone: the same partition as the emitted order's
        base = _ref("noise_as_emitted", lambda: _noise_mesh("as_emitted"))
        assert np.array_equal(np.sort(st["triangles"]), np.sort(base[4]["triangles"]))
        if variant == "triangles_permuted":
            assert np.array_equal(labels, base[2])
    tc = st["triangles"]
    k = 40
    cut = np.sort(tc)[-k]
    assert (tc == cut).sum() > ((tc >= cut).sum() - k) > 0, "the k-th place is tied: the tie rule decides"
    _check_clean(R, key, make, by="triangles", keep_largest=k)
    _check_clean(R, key, make, keep_largest=7)
    _check_clean(R, key, make, min_fraction=1e-4, min_triangles=12)


# ---- union-find and scan adversaries ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(F.SMALL_MESHES))
def test_small_meshes(R, name):
    make = F.SMALL_MESHES[name]
    _check_components(R, name, make)
    _check_clean(R, name, make)
    _check_clean(R, name, make, keep_largest=2)
    _check_clean(R, name, make, by="triangles", min_triangles=2)


def test_empty_meshes(R):
    d = device()
    for V in (0, 5):
        v = torch.zeros(V, 3, dtype=torch.float64, device=d)
        t = torch.zeros(0, 3, dtype=torch.int32, device=d)
        got = R.mesh_components(t, vertices=v)
        assert got["n_components"] == 0 and got["labels"].shape == (V,) and (got["labels"] == -1).all()
        assert got["area"].shape == (0,) and got["bbox_min"].shape == (0, 3) and got["triangles"].shape == (0,)
        for kw in ({}, {"keep_largest": 1}, {"min_fraction": 0.5, "by": "triangles"}):
            out = R.clean_mesh(v, t, attributes={"a": torch.zeros(V, 2, device=d)}, **kw)
            assert out["vertices"].shape == (0, 3) and out["triangles"].shape == (0, 3) and out["vertex_index"].shape == (0,)
            assert out["attributes"]["a"].shape == (0, 2) and out["info"]["n_components"] == 0


def test_a_nan_vertex_in_a_small_component(R):
    def make():
        v, t = F.isolated(5, seed=3)
        v = v.copy()
        v[7, 1] = np.nan                                      # component 2
        return v, t
    v, t, labels, n, st, _ = _ref("nan", make)
    assert np.isnan(st["area"][2]) and np.isnan(st["area"]).sum() == 1 and np.isnan(st["bbox_min"][2, 1])
    got = _check_components(R, "nan", make)
    assert np.isnan(_np(got["area"])[2]) and np.isnan(_np(got["bbox_max"])[2, 1]) and not np.isnan(_np(got["bbox_max"])[2, 0])
    # it ranks below every number
    assert _check_clean(R, "nan", make, keep_largest=4)[1].tolist() == [True, True, False, True, True]
    assert not _check_clean(R, "nan", make, min_fraction=0.0)[1][2]
    assert _check_clean(R, "nan", make, keep_largest=5)[1].all()


@pytest.mark.parametrize("bad", ["V", "-1"])
def test_an_out_of_range_index_is_refused_and_leaves_nothing_behind(R, bad):
    """Argument validation: the kernel checks every index before it uses it as an address, skips the triangle and raises a
    flag; Python turns the flag into ValueError.  The next valid call is exact."""
    v, t, labels, n, st, _ = _ref("A", lambda: _mc_on_device(R, F.volume_a()))
    t_bad = t.copy()
    t_bad[1234, 1] = len(v) if bad == "V" else -1
    with pytest.raises(ValueError, match="outside"):
        R.mesh_components(_dev(t_bad), vertices=_dev(v))
    with pytest.raises(ValueError, match="outside"):
        R.clean_mesh(_dev(v), _dev(t_bad), keep_largest=1)
    _check_components(R, "A", lambda: _mc_on_device(R, F.volume_a()))
    _check_clean(R, "A", lambda: _mc_on_device(R, F.volume_a()), keep_largest=1)


# ---- the renderer ---------------------------------------------------------------------------------------------------
def test_extract_geometry_clean_on_the_geometric_init(R):
    """One component: keep_largest=1 leaves the mesh as it is; clean=None is the unchanged code path (marching cubes + the
    rescale, as tests/test_gpu_mcubes.py has it)."""
    mc = O.ModelConf()
    torch.manual_seed(0)
    p = O.init_params(mc)
    ren = R.build_from_named_params(mc, p, device())[3]
    res = 96
    plain_v, plain_t = ren.extract_geometry(LO, HI, res, threshold=0.0, backend="native")
    assert ren.last_mesh_clean is None
    u = ren.extract_fields(LO, HI, res, to_host=False)
    gv, gt = R.marching_cubes(u, 0.0)
    want_v = _np(gv) / (res - 1.0) * (HI - LO).numpy()[None] + LO.numpy()[None]
    assert np.array_equal(plain_v, want_v) and np.array_equal(plain_t, _np(gt))
    cv, ct = ren.extract_geometry(LO, HI, res, threshold=0.0, backend="native", clean={"keep_largest": 1})
    info = ren.last_mesh_clean
    assert info["n_components"] == 1 and _np(info["kept"]).tolist() == [0] and info["n_triangles"] == (len(gt), len(gt))
    assert cv.dtype == np.float64 and ct.dtype == np.int32
    assert np.array_equal(cv, plain_v) and np.array_equal(ct, plain_t)
    out = R.clean_mesh(_dev(plain_v), _dev(plain_t), keep_largest=1)
    assert np.array_equal(_np(out["vertices"]), cv) and np.array_equal(_np(out["triangles"]), ct)
    cv0, ct0 = ren.extract_geometry(LO, HI, res, threshold=0.0, backend="native", clean={})
    assert np.array_equal(cv0, plain_v) and np.array_equal(ct0, plain_t)


def _floater_threshold(R, ren, res):
    """a level at which the sharp model's iso-surface has more than one component (None when there is none)"""
    u = ren.extract_fields(LO, HI, res, to_host=False)
    for thr in (0.0, 0.05, -0.05, 0.1, -0.1, 0.2, -0.2, 0.3):
        v, t = R.marching_cubes(u, thr)
        if len(t) and R.mesh_components(t, n_vertices=len(v))["n_components"] > 1:
            return thr
    return None


def test_extract_textured_geometry_clean(R, tmp_path):
    ren = U.renderer(R, "sharp", device())
    res = 70
    scale = lambda gv: _np(gv) / (res - 1.0) * (HI - LO).numpy()[None] + LO.numpy()[None]     # noqa: E731
    thr = _floater_threshold(R, ren, res)
    print(f"sharp model at res {res}: " + (f"a fragment splits off at threshold {thr}" if thr is not None
                                           else "one component at every level tried: a small sphere is added"))
    if thr is not None:
        tex = ren.extract_textured_geometry(LO, HI, res, threshold=thr, clean={"keep_largest": 1})
        info = ren.last_mesh_clean
        assert info["n_components"] > 1 and _np(info["kept"]).shape == (1,)
        # its geometry is the cleaned geometry
        geo_v, geo_t = ren.extract_geometry(LO, HI, res, threshold=thr, backend="native", clean={"keep_largest": 1})
        assert np.array_equal(tex["vertices"], geo_v) and np.array_equal(tex["triangles"], geo_t)
        gv, gt = R.marching_cubes(ren.extract_fields(LO, HI, res, to_host=False), thr)
        cleaned = R.clean_mesh(gv, gt, keep_largest=1)
        assert 0 < len(cleaned["vertices"]) < len(gv)
        assert np.array_equal(tex["triangles"], _np(cleaned["triangles"])) and np.array_equal(tex["vertices"], scale(cleaned["vertices"]))
        # removed vertices are never evaluated: the attributes are those of the cleaned vertices alone, bit for bit
        direct = ren.vertex_attributes(grid_vertices=cleaned["vertices"], bounds=(LO, HI), resolution=res, threshold=thr)
        for k_tex, k_at in (("normals", "normal"), ("sdf", "sdf"), ("albedo", "albedo"), ("colors", "rgb")):
            assert np.array_equal(tex[k_tex], _np(direct[k_at])), k_tex
    else:   # no fragment at any level tried: add a small sphere to the model's grid (u = -sdf, so the union is the maximum)
        thr = 0.0
        u = torch.maximum(ren.extract_fields(LO, HI, res, to_host=False),
                          _dev(F.volume_a(res, spheres=(((0.8, 0.8, 0.8), 0.08),))))
        gv, gt = R.marching_cubes(u, thr)
        assert R.mesh_components(gt, vertices=gv)["n_components"] > 1, "the case needs a floater"
        cleaned = R.clean_mesh(gv, gt, keep_largest=1)
        assert 0 < len(cleaned["vertices"]) < len(gv)
        direct = ren.vertex_attributes(grid_vertices=cleaned["vertices"], bounds=(LO, HI), resolution=res, threshold=thr)
        tex = {"vertices": scale(cleaned["vertices"]), "triangles": _np(cleaned["triangles"]), "normals": _np(direct["normal"]),
               "sdf": _np(direct["sdf"]), "albedo": _np(direct["albedo"]), "colors": _np(direct["rgb"])}
    # defaults: clean=None is marching cubes + the rescale + vertex_attributes, as before
    gv, gt = R.marching_cubes(ren.extract_fields(LO, HI, res, to_host=False), 0.0)
    plain = ren.extract_textured_geometry(LO, HI, res)
    assert np.array_equal(plain["triangles"], _np(gt)) and np.array_equal(plain["vertices"], scale(gv))
    full = ren.vertex_attributes(grid_vertices=gv, bounds=(LO, HI), resolution=res)
    for k_tex, k_at in (("normals", "normal"), ("sdf", "sdf"), ("albedo", "albedo"), ("colors", "rgb")):
        assert np.array_equal(plain[k_tex], _np(full[k_at])), k_tex
    # the fp64 oracle under the rule of tests/parity.py, as tests/test_gpu_mesh_attrs.py applies it
    pts = torch.tensor(tex["vertices"]).type(torch.float32)
    assert torch.equal(direct["points"].cpu(), pts)
    ref = U.oracle_attributes("sharp", pts)
    for k in ("sdf", "albedo"):
        P.check_value(f"cleaned textured mesh: {k}", torch.from_numpy(tex[k]), *ref[k])
    g64, g32 = ref["gradient"]
    n64, n32 = (torch.nn.functional.normalize(g, dim=1) for g in (g64, g32))
    P.check_value("cleaned textured mesh: normals", torch.from_numpy(tex["normals"]), n64, n32.double())
    assert np.array_equal(tex["colors"], U.quantize_rgb(torch.from_numpy(tex["albedo"])).numpy())
    # the PLY round trip of the cleaned dict
    path = tmp_path / "clean.ply"
    R.write_ply(path, tex["vertices"], tex["triangles"], normals=tex["normals"], colors=tex["colors"])
    m = R.read_ply(path)
    assert np.array_equal(m["vertices"], tex["vertices"].astype(np.float32)) and np.array_equal(m["triangles"], tex["triangles"])
    assert np.array_equal(m["normals"], tex["normals"]) and np.array_equal(m["colors"], tex["colors"])
