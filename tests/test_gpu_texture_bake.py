"""Texture baking on the device (`rnb_texture_sample_points`, `rnb_texture_pack`, `NeuSRenderer.bake_textures`,
`extract_textured_geometry(bake=)`, `sample_texture`) against the numpy restatement tests/texture_bake_ref.py — bit for
bit for everything the atlas defines (sample points, texel map, both images) — and against the CPU oracle for what the
field contributes.

Bounds.  fp32 route: `tests/parity.check_value` against the fp32 and fp64 oracle at the device's own fp32 sample points,
the rule of tests/test_gpu_mesh_attrs.py; nothing hand-set.  bf16 route: the project's stated point-wise bf16 bounds against
the fp32 oracle (SDF_ATOL, NRM_ATOL, OUT_ATOL = 1e-2, 1e-1, 3e-2, as quoted in tests/test_gpu_mesh_attrs.py).  The camera
and Newton tests print their figures and assert only the strict decrease.  The end-to-end mesh (the `sharp` model at
resolution 70, clustered at 3 voxels, chart 4: about 1,450 triangles, 22,000 samples) is baked once and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import rnb_oracle as O
from tests import mesh_attrs_util as U
from tests import mesh_raycast_ref as MR
from tests import parity as P
from tests import texture_bake_ref as F
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device

pytestmark = pytest.mark.gpu

LO, HI = U.LO, U.HI
SDF_ATOL, NRM_ATOL, OUT_ATOL = 1e-2, 1e-1, 3e-2      # tests/test_gpu_mesh_attrs.py: bf16 point-wise SDF, normal, outputs
RES, CELL, CHART = 70, 3, 4
N_ORACLE = 2000                                      # samples the CPU oracle evaluates per check


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device())


def _np(x):
    return x.detach().cpu().numpy()


def _meshes():
    ico_v, ico_t = MR.icosphere(1)
    quad = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [0.0, 1.0, -0.5], [1.0, 1.0, 0.125], [2.0, 0.5, 0.75]])
    bad_v = np.concatenate([quad, [[0.5, np.nan, 0.0]]])
    return {
        "one": (quad[:3], np.array([[0, 1, 2]], dtype=np.int32)),
        "two": (quad[:4], np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32)),
        "three": (quad, np.array([[0, 1, 2], [2, 1, 3], [1, 4, 3]], dtype=np.int32)),
        "ico": (ico_v, ico_t),
        # triangle 1 names vertex 6 of 6, triangle 3 has the NaN corner
        "bad": (bad_v, np.array([[0, 1, 2], [2, 6, 3], [1, 4, 3], [0, 5, 1], [2, 1, 3]], dtype=np.int32)),
    }


MESHES = _meshes()


def _sample_points(R, v, t, s, first, count):
    """(points [count,3] float32 as numpy, the bad counter) of one rnb_texture_sample_points call"""
    vd, td = _dev(v), _dev(t)
    pts = torch.full((count, 3), float("nan"), dtype=torch.float32, device=device())
    bad = torch.zeros(1, dtype=torch.int64, device=device())
    lib = R.native.load()
    with R.native.on_device(vd) as stream:
        R.native.check(lib.rnb_texture_sample_points(R.native.ptr(vd), len(v), R.native.ptr(td), len(t), s, first, count,
                                                     R.native.ptr(pts), R.native.ptr(bad), stream))
    return _np(pts), int(bad.cpu())


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("s", [1, 2, 7])
@pytest.mark.parametrize("name", ["one", "two", "three", "ico", "bad"])
def test_sample_points_match_the_reference_bit_for_bit(R, name, s):
    v, t = MESHES[name]
    n_s = F.n_samples(s)
    N = len(t) * n_s
    want, want_bad = F.sample_points(v, t, s)
    got, bad = _sample_points(R, v, t, s, 0, N)
    assert _same_bits(got, want), f"{name} s={s}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} words differ"
    assert bad == want_bad == (2 if name == "bad" else 0)
    if name == "bad":
        z = got.reshape(len(t), n_s, 3)
        assert not z[1].any() and not z[3].any() and np.isfinite(got).all(), "bad triangles put their samples at the origin"
    # ranges: first inside a triangle, one sample, a range ending at the last sample, a range ending inside a triangle
    ranges = [(1, N - 1), (N - 1, 1), (0, 1), (n_s // 2 + 1, min(N - n_s // 2 - 1, n_s + 2)), (max(N - n_s - 1, 0), min(n_s + 1, N))]
    total_bad = 0
    for first, count in ranges:
        part, b = _sample_points(R, v, t, s, first, count)
        ref, ref_b = F.sample_points(v, t, s, first, count)
        assert _same_bits(part, ref) and _same_bits(part, want[first:first + count]) and b == ref_b, (name, s, first, count)
        total_bad += b
    # a partition of the whole set counts every bad triangle once
    cuts = sorted({0, 1, n_s - 1, n_s, N // 2, N})
    assert sum(_sample_points(R, v, t, s, a, b - a)[1] for a, b in zip(cuts[:-1], cuts[1:]) if b > a) == want_bad


@pytest.mark.parametrize("s", [1, 2, 7])
def test_corner_samples_are_the_vertices_and_shared_edges_agree(R, s):
    v, t = MESHES["ico"]
    n_s = F.n_samples(s)
    got, _ = _sample_points(R, v, t, s, 0, len(t) * n_s)
    P3 = got.reshape(len(t), n_s, 3)
    corners = [int(F.rank(s, 0, 0)), int(F.rank(s, s, 0)), int(F.rank(s, 0, s))]
    assert (P3[:, corners] == v[t].astype(np.float32)).all(), "a corner sample is its vertex converted to fp32"
    # the lattice points of every edge, ordered from the smaller vertex index to the larger, from both triangles
    m = np.arange(s + 1)
    edge_rank = [F.rank(s, m, 0 * m), F.rank(s, s - m, m), F.rank(s, 0 * m, s - m)]      # corner k -> corner k + 1
    seen = {}
    for ti in range(len(t)):
        for k in range(3):
            a, b = int(t[ti, k]), int(t[ti, (k + 1) % 3])
            pts = P3[ti, edge_rank[k]]
            seen.setdefault((min(a, b), max(a, b)), []).append(pts if a < b else pts[::-1])
    assert len(seen) == 120 and all(len(x) == 2 for x in seen.values()), "a closed surface: every edge has two triangles"
    for (a, b), (p, q) in seen.items():
        assert (p == q).all(), f"edge {a}-{b}: the two sides disagree"
    if s > 1:
        assert len(np.unique(P3.reshape(-1, 3), axis=0)) == 42 + 120 * (s - 1) + 80 * (n_s - 3 * s), "and nothing else coincides"


def _pack(R, v, t, L, rgb, normal, outputs=(True, True, True)):
    vd, td = _dev(v), _dev(t)
    a, n, ts = R.runtime.texture_pack(vd, td, L["s"], L["cols"], L["W"], L["H"], None if rgb is None else _dev(rgb),
                                      None if normal is None else _dev(normal), albedo=outputs[0], normals=outputs[1],
                                      texel_sample=outputs[2])
    return tuple(None if x is None else _np(x) for x in (a, n, ts))


def _synthetic(N, seed):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (N, 3), dtype=np.uint8)
    nrm = rng.uniform(-1.3, 1.3, (N, 3)).astype(np.float32)
    special = np.array([0.0, -0.0, 1.0, -1.0, 1.0 / 255.0, -1.0 / 255.0, 0.5, 2.0, -2.0, np.inf, -np.inf, np.nan,
                        3.0 / 255.0, np.float32(1.0) - np.float32(2.0 ** -24)], dtype=np.float32)
    k = min(len(special), nrm.size)
    nrm.reshape(-1)[:k] = special[:k]
    return rgb, nrm


@pytest.mark.parametrize("s", [1, 2, 7])
@pytest.mark.parametrize("name", ["one", "two", "three", "ico", "bad"])
def test_pack_matches_the_reference(R, name, s):
    v, t = MESHES[name]
    T = len(t)
    N = T * F.n_samples(s)
    rgb, nrm = _synthetic(N, 10 * s + T)
    bad = F.bad_triangles(v, t)
    chosen = F.layout(T, chart=s)
    forced = F.layout(T, size=chosen["W"] + s + 8, chart=s)          # margins right of the cells and below them
    assert forced["W"] > forced["cols"] * forced["c"] or forced["cols"] > chosen["cols"]
    for L in (chosen, forced):
        assert R.atlas_layout(T, size=None if L is chosen else L["W"], chart=s).asdict() == L
        a_img, n_img, smp = _pack(R, v, t, L, rgb, nrm)
        wa, wn, ws = F.pack(L, v, t, rgb, nrm)
        assert smp.dtype == np.int32 and np.array_equal(smp, ws)
        assert a_img.shape == (L["H"], L["W"], 4) and np.array_equal(a_img, wa) and np.array_equal(n_img, wn)
        live = smp >= 0
        assert not a_img[~live].any() and not n_img[~live].any(), "empty texels are all zero"
        assert (a_img[live][:, 3] == 255).all() and (n_img[live][:, 3] == 255).all()
        _, owner = F.texel_map(L, T)
        good = np.isin(owner, np.flatnonzero(~bad))
        assert np.array_equal(live, good), "the non-empty texels are the owned texels of the good triangles"
        assert np.array_equal(a_img[live][:, :3], rgb[smp[live]])
        assert np.array_equal(n_img[live][:, :3], F.quantize_normal(nrm)[smp[live]])
        assert set(np.unique(smp[live])) == set(np.flatnonzero(np.repeat(~bad, F.n_samples(s)))), "every sample has a texel"
    # each output alone
    only_a = _pack(R, v, t, chosen, rgb, None, (True, False, False))
    only_n = _pack(R, v, t, chosen, None, nrm, (False, True, False))
    only_s = _pack(R, v, t, chosen, None, None, (False, False, True))
    wa, wn, ws = F.pack(chosen, v, t, rgb, nrm)
    assert np.array_equal(only_a[0], wa) and np.array_equal(only_n[1], wn) and np.array_equal(only_s[2], ws)
    assert only_a[1] is None and only_a[2] is None


def test_normal_quantisation_special_values(R):
    """zero gives 128, +-1 give 255 / 0, out of range clips, NaN gives 0: on the device as in the reference"""
    v, t = MESHES["one"]
    s = 7
    N = F.n_samples(s)
    _, nrm = _synthetic(N, 0)
    q = F.quantize_normal(nrm)
    assert q.reshape(-1)[:12].tolist() == [128, 128, 255, 0, 128, 127, 191, 255, 0, 255, 0, 0]
    L = F.layout(1, chart=s)
    _, n_img, smp = _pack(R, v, t, L, None, nrm, (False, True, True))
    assert np.array_equal(n_img[smp >= 0][:, :3], q[smp[smp >= 0]])
    # T == 0: the outputs are cleared without a kernel
    a_img, n_img, smp = _pack(R, v, np.zeros((0, 3), dtype=np.int32), dict(s=2, c=7, cols=0, W=9, H=5), None, None)
    assert not a_img.any() and not n_img.any() and (smp == -1).all() and smp.shape == (5, 9)


# ---- end to end ---------------------------------------------------------------------------------------------------------

_E2E = {}


def _baked(R):
    """the shared end-to-end result (device tensors); callers must not modify it"""
    if "tex" not in _E2E:
        ren = U.renderer(R, "sharp", device())
        _E2E["tex"] = ren.extract_textured_geometry(LO, HI, RES, to_host=False, simplify={"cell_size": CELL},
                                                    bake={"chart": CHART, "return_samples": True})
        torch.cuda.synchronize()
    return _E2E["tex"]


def _subsample(N, seed=0):
    return torch.from_numpy(np.sort(np.random.default_rng(seed).choice(N, min(N, N_ORACLE), replace=False)))


def _check_samples(tag, bake, idx):
    """sdf, unit normal and albedo of the samples `idx` against the oracle at the device's own fp32 points"""
    pts = bake["points"].cpu()[idx]
    ref = U.oracle_attributes("sharp", pts)
    g64, g32 = ref["gradient"]
    n64, n32 = (torch.nn.functional.normalize(g, dim=1) for g in (g64, g32))
    checks = [("sdf", bake["sdf"].cpu()[idx], *ref["sdf"]), ("normal", bake["normal"].cpu()[idx], n64, n32.double())]
    if "albedo" in bake:
        checks.append(("albedo", bake["albedo"].cpu()[idx], *ref["albedo"]))
    for k, got, r64, r32 in checks:
        e_dev, e_ref, bound = P.value_errors(got, r64, r32)
        print(f"{tag}: {k} |dev - fp64| {e_dev:.3e}, fp32 oracle {e_ref:.3e}, bound {bound:.3e}")
    for k, got, r64, r32 in checks:
        P.check_value(f"{tag}: {k}", got, r64, r32)


def test_end_to_end_samples_match_the_oracle_and_images_the_reference_pack(R):
    tex = _baked(R)
    bake = tex["bake"]
    v, t = tex["vertices"], tex["triangles"]
    T = t.shape[0]
    lay = bake["layout"]
    assert set(tex) == {"vertices", "triangles", "normals", "sdf", "albedo", "colors", "uv", "albedo_image", "normal_image", "bake"}
    assert set(bake) == {"texel_sample", "layout", "info", "points", "sdf", "normal", "albedo"}
    assert 500 < T < 5000 and lay == R.atlas_layout(T, chart=CHART) and lay.samples_per_triangle == 15
    N = T * 15
    assert bake["info"] == {"samples": N, "bad_triangles": 0, "slabs": 1}
    assert bake["points"].shape == (N, 3) and bake["sdf"].shape == (N, 1) and bake["albedo"].shape == (N, 3)
    assert tex["albedo_image"].shape == (lay.H, lay.W, 4) and tex["albedo_image"].dtype == torch.uint8 and tex["albedo_image"].is_cuda
    # the sample points are the reference's lattice of the final vertices, and uv is atlas_uv
    want_pts, _ = F.sample_points(_np(v), _np(t), CHART)
    assert _same_bits(_np(bake["points"]), want_pts)
    assert tex["uv"].dtype == torch.float64 and np.array_equal(_np(tex["uv"]), R.atlas_uv(lay, T))
    _check_samples("bake chart 4", bake, _subsample(N))
    # the images are the reference pack of the returned samples
    rgb = U.quantize_rgb(bake["albedo"]).numpy()
    wa, wn, ws = F.pack(lay.asdict(), _np(v), _np(t), rgb, _np(bake["normal"]))
    assert np.array_equal(_np(bake["texel_sample"]), ws)
    assert np.array_equal(_np(tex["albedo_image"]), wa) and np.array_equal(_np(tex["normal_image"]), wn)
    assert float(_np(tex["albedo_image"])[ws >= 0][:, :3].std()) > 1.0, "degenerate colours"
    nn = _np(bake["normal"])
    assert np.abs(np.linalg.norm(nn, axis=1) - 1.0).max() < 1e-5


def test_two_calls_and_two_slab_sizes_give_the_same_bits(R):
    tex = _baked(R)
    ren = U.renderer(R, "sharp", device())
    v, t = tex["vertices"], tex["triangles"]
    N = t.shape[0] * 15
    first = {**{k: tex[k] for k in ("uv", "albedo_image", "normal_image")}, **tex["bake"]}
    for slab in (1 << 20, 64 * 16, 64 * 100):
        again = ren.bake_textures(v, t, chart=CHART, return_samples=True, to_host=False, slab=slab)
        assert again["info"]["slabs"] == -(-N // slab) and again["info"]["samples"] == N
        for k in ("uv", "albedo_image", "normal_image", "texel_sample", "points", "sdf", "normal", "albedo"):
            assert torch.equal(first[k], again[k]), f"slab {slab}: {k} differs"
    # to_host: the same arrays as numpy
    host = ren.bake_textures(v, t, chart=CHART)
    assert set(host) == {"uv", "albedo_image", "normal_image", "texel_sample", "layout", "info"}
    for k in ("uv", "albedo_image", "normal_image", "texel_sample"):
        assert isinstance(host[k], np.ndarray) and np.array_equal(host[k], _np(first[k])), k


def test_bake_none_leaves_the_method_as_it_is(R):
    tex = _baked(R)
    ren = U.renderer(R, "sharp", device())
    plain = ren.extract_textured_geometry(LO, HI, RES, to_host=False, simplify={"cell_size": CELL}, bake=None)
    default = ren.extract_textured_geometry(LO, HI, RES, to_host=False, simplify={"cell_size": CELL})
    assert set(plain) == set(default) == {"vertices", "triangles", "normals", "sdf", "albedo", "colors"}
    for k in plain:
        assert torch.equal(plain[k], default[k]) and torch.equal(plain[k], tex[k]), k
    # to_host with a bake: numpy everywhere, the same images
    host = ren.extract_textured_geometry(LO, HI, RES, simplify={"cell_size": CELL}, bake={"chart": CHART})
    assert set(host["bake"]) == {"texel_sample", "layout", "info"}
    for k in ("uv", "albedo_image", "normal_image"):
        assert isinstance(host[k], np.ndarray) and np.array_equal(host[k], _np(tex[k])), k
    assert np.array_equal(host["vertices"], _np(tex["vertices"])), "the host's rescaling equals the device's here"


def test_what_a_camera_sees(R, tmp_path):
    """A 48 x 48 pinhole view of the simplified mesh: the fp32 oracle's albedo at the hit points against (a) the baked float
    albedo, gathered through texel_sample and looked up with sample_texture, and (b) the per-vertex albedo interpolated
    by MeshIndex.interpolate.  Confirmed beforehand on the CPU with the oracle alone (numpy marching cubes, clustering,
    lattice and lookup of the test references) at cell_size = 3 voxels, chart = 4, this view: mean |error| 6.8e-4 baked
    against 3.0e-3 per vertex (1.1e-3 against 3.6e-3 from a second eye), so the issue's shapes are used as they are.  Both
    errors are printed; only `baked < per-vertex` is asserted."""
    tex = _baked(R)
    bake = tex["bake"]
    v, t = tex["vertices"], tex["triangles"]
    index = R.MeshIndex(v, t)
    o, d = MR.pinhole_rays(48, 48, [0.0, -2.4, 0.5], [0.0, 0.0, 0.0], 40.0)
    hits = index.raycast(_dev(o), _dev(d))
    hit = hits["hit"].cpu()
    assert int(hit.sum()) > 400
    mc, p, _ = U.model("sharp")
    truth = U.attributes(p, mc, hits["point"].cpu()[hit].float())[2].double()
    smp = bake["texel_sample"]
    image = torch.where((smp >= 0)[..., None], bake["albedo"][smp.clamp(min=0).long()], torch.zeros((), device=device()))
    baked = R.sample_texture(image, tex["uv"], hits["triangle"], hits["bary"]).cpu()
    assert bool(torch.isnan(baked[~hit]).all()) and bool(torch.isfinite(baked[hit]).all())
    vertex = index.interpolate(hits, tex["albedo"]).cpu()[hit].double()
    e_baked, e_vertex = float((baked[hit] - truth).abs().mean()), float((vertex - truth).abs().mean())
    print(f"camera 48x48, {int(hit.sum())} hits: mean |albedo error| baked {e_baked:.3e}, per vertex {e_vertex:.3e} "
          f"(ratio {e_vertex / max(e_baked, 1e-300):.2f})")
    assert e_baked < e_vertex
    # the uint8 image: at texel centres it is quantize_rgb of the float samples
    live = (smp >= 0).cpu()
    a_img = tex["albedo_image"].cpu()
    want = U.quantize_rgb(bake["albedo"].cpu()[smp.cpu()[live].long()])
    assert torch.equal(a_img[live][:, :3], want) and bool((a_img[live][:, 3] == 255).all())
    T = t.shape[0]
    corner = R.sample_texture(tex["albedo_image"][..., :3], tex["uv"], torch.arange(T, device=device()).repeat_interleave(3),
                              torch.eye(3, dtype=torch.float64, device=device()).repeat(T, 1)).cpu()
    ranks = torch.tensor([int(F.rank(CHART, 0, 0)), int(F.rank(CHART, CHART, 0)), int(F.rank(CHART, 0, CHART))])
    at = (torch.arange(T)[:, None] * 15 + ranks[None]).reshape(-1)
    assert float((corner - U.quantize_rgb(bake["albedo"].cpu()[at]).double()).abs().max()) < 1e-6
    # and the export: OBJ + MTL + two PNGs read back as written
    host = {k: _np(tex[k]) for k in ("vertices", "triangles", "uv", "normals", "albedo_image", "normal_image")}
    R.write_png(tmp_path / "m_albedo.png", host["albedo_image"])
    R.write_png(tmp_path / "m_normal.png", host["normal_image"])
    R.write_obj(tmp_path / "m.obj", host["vertices"], host["triangles"], host["uv"], normals=host["normals"],
                material={"albedo": "m_albedo.png", "normal": "m_normal.png"})
    m = R.read_obj(tmp_path / "m.obj")
    assert np.array_equal(m["vertices"], host["vertices"]) and np.array_equal(m["uv"], host["uv"])
    assert np.array_equal(R.read_png(tmp_path / m["material"]["albedo"]), host["albedo_image"])
    assert np.array_equal(R.read_png(tmp_path / m["material"]["normal"]), host["normal_image"])


def test_one_newton_step_moves_the_samples_towards_the_level_set(R):
    tex = _baked(R)
    ren = U.renderer(R, "sharp", device())
    mc, _, p64 = U.model("sharp")
    v, t = tex["vertices"], tex["triangles"]
    step = float(((HI - LO).double() / (RES - 1)).pow(2).sum().sqrt())
    with pytest.raises(ValueError, match="max_step"):
        ren.bake_textures(v, t, chart=CHART, refine=1)
    moved = ren.bake_textures(v, t, chart=CHART, refine=1, max_step=step, return_samples=True, to_host=False)
    p0, p1 = tex["bake"]["points"].cpu().double(), moved["points"].cpu().double()
    dist = (p1 - p0).norm(dim=1)
    assert float(dist.max()) <= step * (1 + 1e-6) and float(dist.max()) > 0.0
    idx = _subsample(p0.shape[0], seed=1)
    rms = []
    for pts in (p0, p1):
        with torch.no_grad():
            f = O.sdf_only(p64, mc.sdf, pts[idx])[:, 0]
        rms.append(float(f.pow(2).mean().sqrt()))
    print(f"rms |sdf| over {len(idx)} samples: refine=0 {rms[0]:.3e}, refine=1 {rms[1]:.3e} (ratio {rms[0] / max(rms[1], 1e-300):.1f}); "
          f"largest move {float(dist.max()):.3e} (max_step {step:.3e})")
    assert rms[1] < rms[0]
    _check_samples("bake refine=1", moved, idx)
    # through the extract call: max_step defaults to one cell diagonal, and the bake follows the refined vertices
    both = ren.extract_textured_geometry(LO, HI, RES, to_host=False, refine=1, simplify={"cell_size": CELL},
                                         bake={"chart": CHART, "refine": 1, "return_samples": True})
    want_pts, _ = F.sample_points(_np(both["vertices"]), _np(both["triangles"]), CHART)
    d2 = (both["bake"]["points"].cpu().double() - torch.from_numpy(want_pts).double()).norm(dim=1)
    assert float(d2.max()) <= step * (1 + 1e-6)
    assert not torch.equal(both["vertices"], tex["vertices"])


def test_renderer_without_the_albedo_network(R):
    mc, p, _ = U.model("tiny")
    sdf, dev, col, full = R.build_from_named_params(mc, p, device())
    geo = R.NeuSRenderer(None, sdf, dev, None, n_samples=16, n_importance=16, n_outside=0, up_sample_steps=4, perturb=0.0)
    v, t = MESHES["ico"]
    vd, td = _dev(v * 0.5), _dev(t)
    out = geo.bake_textures(vd, td, chart=2, return_samples=True, to_host=False)
    assert out["albedo_image"] is None and "albedo" not in out
    assert out["normal_image"].shape == (out["layout"].H, out["layout"].W, 4)
    wa, wn, ws = F.pack(out["layout"].asdict(), v * 0.5, t, None, _np(out["normal"]))
    assert wa is None and np.array_equal(_np(out["normal_image"]), wn) and np.array_equal(_np(out["texel_sample"]), ws)
    with pytest.raises(ValueError, match="albedo"):
        geo.bake_textures(vd, td, chart=2, albedo=True)
    # albedo=False on a full renderer: the same normal image
    plain = full.bake_textures(vd, td, chart=2, albedo=False, to_host=False)
    assert plain["albedo_image"] is None and torch.equal(plain["normal_image"], out["normal_image"])
    # a bad triangle is reported and its texels are empty; an empty mesh bakes to empty images
    bv, bt = MESHES["bad"]
    bad = full.bake_textures(_dev(np.nan_to_num(bv, nan=np.inf) * 0.3), _dev(bt), chart=2, to_host=False)
    assert bad["info"]["bad_triangles"] == 2
    n_s = F.n_samples(2)
    assert set(np.unique(_np(bad["texel_sample"]) // n_s)) == {-1, 0, 2, 4}
    empty = full.bake_textures(vd, td[:0], chart=2)
    assert empty["albedo_image"].shape == (0, 0, 4) and empty["uv"].shape == (0, 3, 2) and empty["info"]["samples"] == 0


def test_bf16_route(R):
    tex = _baked(R)
    ren = U.renderer(R, "sharp_bf16", device())
    v, t = tex["vertices"], tex["triangles"]
    a = ren.bake_textures(v, t, chart=CHART, return_samples=True, to_host=False)
    b = ren.bake_textures(v, t, chart=CHART, return_samples=True, to_host=False)
    for k in ("albedo_image", "normal_image", "texel_sample", "points", "sdf", "normal", "albedo"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["points"], tex["bake"]["points"]) and torch.equal(a["texel_sample"], tex["bake"]["texel_sample"])
    live = a["texel_sample"] >= 0
    assert bool((a["albedo_image"][live][:, 3] == 255).all()) and bool((a["normal_image"][live][:, 3] == 255).all())
    idx = _subsample(a["points"].shape[0], seed=2)
    ref = U.oracle_attributes("sharp", a["points"].cpu()[idx])
    n32 = torch.nn.functional.normalize(ref["gradient"][1], dim=1)
    errs = {"sdf": float((a["sdf"].cpu()[idx] - ref["sdf"][1]).abs().max()),
            "normal": float((a["normal"].cpu()[idx] - n32).abs().max()),
            "albedo": float((a["albedo"].cpu()[idx] - ref["albedo"][1]).abs().max())}
    print("bf16 bake vs the fp32 oracle: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert errs["sdf"] <= SDF_ATOL and errs["normal"] <= NRM_ATOL and errs["albedo"] <= OUT_ATOL
