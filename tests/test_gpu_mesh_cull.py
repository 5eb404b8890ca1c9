"""Mesh culling on the device against tests/mesh_cull_ref.py: the status of every (camera, point) pair and the votes of
rnb_mesh_view_votes BIT FOR BIT, the SEEN / OCCLUDED split against `MeshIndex.visible`, the edges of the rule, the
compaction by a per-triangle keep, `cull_mesh`, and the renderer's `cull=` keyword.  Everything here is integer or
bit-exact fp64: nothing is held to less than equality."""
import os

import numpy as np
import pytest
import torch

from tests import mesh_cull_ref as F
from tests import mesh_distance_ref as MD
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDENT = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
OUTER_V, OUTER_T, INNER_V, INNER_T = 642, 1280, 162, 320


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device())


def _np(x):
    return x.detach().cpu().numpy()


_DEVICE_SCENE = {}


def _scene(R):
    """the shared scene on the device with its default MeshIndex, once"""
    if not _DEVICE_SCENE:
        s = F.scene()
        d = {k: _dev(s[k]) for k in ("vertices", "triangles", "projections", "eyes", "masks")}
        d["index"] = R.MeshIndex(d["vertices"], d["triangles"])
        d["masks255"] = d["masks"] * 255                                  # a mask IMAGE, as cull_mesh takes it (binary_masks: > 127.5)
        _DEVICE_SCENE.update(d)
    return F.scene(), _DEVICE_SCENE


def _assert_votes(got, status, counts, tag):
    assert got["counts"].dtype == torch.int32 and got["counts"].shape == counts.shape, tag
    assert np.array_equal(_np(got["counts"]), counts), f"{tag}: counts differ in {(_np(got['counts']) != counts).sum()} places"
    for k, name in enumerate(("out_of_frame", "outside_mask", "occluded", "seen")):
        assert got[name].shape == counts[:, k].shape and np.array_equal(_np(got[name]), counts[:, k]), (tag, name)
        if counts.shape[0]:      # a view of the one [N,4] tensor (an empty tensor has no address to compare)
            assert got[name].data_ptr() == got["counts"].data_ptr() + 4 * k and got[name].stride() == (4,), (tag, name)
    if status is not None:
        assert got["status"].dtype == torch.uint8 and np.array_equal(_np(got["status"]), status), f"{tag}: status differs"


# --------------------------------------------------------------------------------------------------------------------- votes
def test_votes_on_the_scene_are_the_reference_bit_for_bit(R):
    s, d = _scene(R)
    got = d["index"].view_votes(d["vertices"], d["projections"], d["eyes"], d["masks"], return_status=True)
    _assert_votes(got, s["status"], s["counts"], "scene")
    assert bool((got["counts"].sum(dim=1) == 6).all())
    assert "status" not in d["index"].view_votes(d["vertices"], d["projections"], d["eyes"], d["masks"])
    # the SEEN / OCCLUDED split of camera c is MeshIndex.visible's answer for eye c
    for c in range(6):
        vis = _np(d["index"].visible(d["vertices"], d["eyes"][c]))
        st = s["status"][c]
        cast = st >= 2
        assert cast.sum() > 300 and np.array_equal(st[cast] == F.SEEN, vis[cast]), f"camera {c}"
    # whatever the grid
    one = R.MeshIndex(d["vertices"], d["triangles"], cells=1)
    _assert_votes(one.view_votes(d["vertices"], d["projections"], d["eyes"], d["masks"], return_status=True), s["status"],
                  s["counts"], "cells=1")
    # without masks, without occlusion, and again (bit-reproducible: integer atomics)
    _assert_votes(d["index"].view_votes(d["vertices"], d["projections"], d["eyes"], image_size=(48, 48)), None, s["counts_nomask"], "no masks")
    _assert_votes(d["index"].view_votes(d["vertices"], d["projections"], d["eyes"], d["masks"], occlusion=False), None,
                  s["counts_noocc"], "no occlusion")
    _assert_votes(d["index"].view_votes(d["vertices"], d["projections"], d["eyes"], d["masks"], return_status=True), s["status"],
                  s["counts"], "second run")
    # rel_tol = 0: the point's own triangle may hide it, never the other way round
    tight = d["index"].view_votes(d["vertices"], d["projections"], d["eyes"], d["masks"], rel_tol=0.0)
    assert bool((tight["seen"] <= got["seen"]).all()) and bool((tight["counts"].sum(dim=1) == 6).all())
    assert np.array_equal(_np(tight["counts"][:, :2]), s["counts"][:, :2])


@pytest.mark.parametrize("N,cams", [(1, 6), (65, 6), (816, 1), (300, 0), (0, 6)])
def test_votes_sizes(R, N, cams):
    """one point, one point past a wavefront, one camera, no camera (zero counts), no point"""
    s, d = _scene(R)
    pick = np.arange(N) * 5 % 816 if N < 816 else np.arange(816)
    pts = d["vertices"][torch.from_numpy(pick).to(device())] if N else d["vertices"][:0]
    got = d["index"].view_votes(pts, d["projections"][:cams], d["eyes"][:cams], d["masks"][:cams], return_status=True)
    status = s["status"][:cams][:, pick]
    counts = np.stack([(status == k).sum(axis=0) for k in range(4)], axis=1).astype(np.int32).reshape(N, 4)
    _assert_votes(got, status, counts, f"N={N} C={cams}")
    assert got["status"].shape == (cams, N)


def test_edges_of_the_rule(R):
    """P = [I | 0] on a 5 x 7 frame and an index with no triangle: u = X exactly, every pair in frame and mask is SEEN"""
    H, W = 5, 7
    edge = [-0.5, np.nextafter(-0.5, -1.0), np.nextafter(-0.5, 1.0), W - 0.5, np.nextafter(W - 0.5, 0.0), np.nextafter(W - 0.5, 10.0)]
    pts = [[u, 1.0, 1.0] for u in edge] + [[1.0, v, 1.0] for v in (-0.5, np.nextafter(-0.5, -1.0), H - 0.5, np.nextafter(H - 0.5, 0.0))]
    pts += [[2.0, 3.0, 1.0], [4.0, 6.0, 2.0], [0.0, 0.0, 0.0], [1.0, 1.0, -1.0], [np.nan, 1.0, 1.0], [1.0, np.inf, 1.0],
            [1.0, 1.0, np.inf], [1.0, 1.0, -np.inf], [3.0, 3.0, 3.0], [1e308, 1e308, 1e-300], [6.0, 4.0, 1.0]]
    pts = np.array(pts)
    mask = np.ones((1, H, W), dtype=np.uint8)
    mask[0, 3, 2] = 0                                                     # where (2, 3, 1) and (4, 6, 2) project
    eye = np.array([[3.0, 3.0, 3.0]])                                     # one of the points IS the eye
    no_v, no_t = np.zeros((3, 3)), np.zeros((0, 3), dtype=np.int32)
    empty = R.MeshIndex(_dev(no_v), _dev(no_t))
    assert empty.n_entries == 0
    want_st, want_c = F.view_votes(pts, IDENT[None], eye, mask, (H, W), no_v, no_t)
    assert want_st[0, :6].tolist() == [3, 0, 3, 0, 3, 0] and want_st[0, 6:10].tolist() == [3, 0, 0, 3]
    assert want_st[0, 10:].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, F.OCCLUDED, 0, 3]
    got = empty.view_votes(_dev(pts), _dev(IDENT[None]), _dev(eye), _dev(mask), return_status=True)
    _assert_votes(got, want_st, want_c, "edges")
    # no masks: the two masked pixels are seen; no occlusion: the point that is the eye is seen too
    st, c = F.view_votes(pts, IDENT[None], eye, None, (H, W), no_v, no_t)
    assert st[0, 10:12].tolist() == [3, 3]
    _assert_votes(empty.view_votes(_dev(pts), _dev(IDENT[None]), _dev(eye), image_size=(H, W), return_status=True), st, c, "edges, no masks")
    st, c = F.view_votes(pts, IDENT[None], eye, mask, (H, W), no_v, no_t, occlusion=False)
    assert st[0, 18] == F.SEEN
    _assert_votes(empty.view_votes(_dev(pts), _dev(IDENT[None]), _dev(eye), _dev(mask), occlusion=False, return_status=True), st, c,
                  "edges, no occlusion")
    # float32 points are widened exactly
    with np.errstate(over="ignore"):
        p32 = pts.astype(np.float32)                                      # (1e308 becomes +inf)
    st, c = F.view_votes(p32.astype(np.float64), IDENT[None], eye, mask, (H, W), no_v, no_t)
    _assert_votes(empty.view_votes(_dev(p32), _dev(IDENT[None]), _dev(eye), _dev(mask), return_status=True), st, c, "float32 points")


def test_occlusion_on_two_parallel_triangles(R):
    v = np.array([[-4.0, -4.0, 2.0], [8.0, -4.0, 2.0], [-4.0, 8.0, 2.0], [-0.25, -0.25, 1.0], [0.5, -0.25, 1.0], [-0.25, 0.5, 1.0]])
    t = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)
    P = np.array([[[10.0, 0.0, 8.0, 0.0], [0.0, 10.0, 8.0, 0.0], [0.0, 0.0, 1.0, 1.0]]])      # w = Z + 1: the eye is in frame
    pts = np.array([[0.0, 0.0, 2.0], [1.0, 1.0, 2.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.1, 0.1, 2.0], [0.1, 0.1, 0.5]])
    eye = np.zeros((1, 3))
    index = R.MeshIndex(_dev(v), _dev(t))
    for occ in (True, False):
        st, c = F.view_votes(pts, P, eye, None, (16, 16), v, t, occlusion=occ)
        if occ:
            assert st[0].tolist() == [F.OCCLUDED, F.SEEN, F.SEEN, F.OCCLUDED, F.OCCLUDED, F.SEEN]
        else:
            assert (st == F.SEEN).all()
        _assert_votes(index.view_votes(_dev(pts), _dev(P), _dev(eye), image_size=(16, 16), occlusion=occ, return_status=True), st, c,
                      f"two triangles, occlusion={occ}")
    with pytest.raises(ValueError, match="without grid="):
        R.MeshIndex(_dev(v), _dev(t), grid=((0.0, 0.0, 0.0), 0.5, (2, 2, 2))).view_votes(_dev(pts), _dev(P), _dev(eye), image_size=(16, 16))


# ---------------------------------------------------------------------------------------------------------------- compaction
def _assert_compaction(got, want, tag):
    v, t, vi, ti = want
    assert got["vertices"].dtype == torch.float64 and got["triangles"].dtype == torch.int32, tag
    assert got["vertex_index"].dtype == torch.int64 and got["triangle_index"].dtype == torch.int64, tag
    assert np.array_equal(_np(got["vertices"]).view(np.uint64), v.view(np.uint64)) and _np(got["vertices"]).shape == v.shape, tag
    assert np.array_equal(_np(got["triangles"]), t) and _np(got["triangles"]).shape == t.shape, tag
    assert np.array_equal(_np(got["vertex_index"]), vi) and np.array_equal(_np(got["triangle_index"]), ti), tag


def test_compact_triangles_on_the_torus(R):
    v, t = MD.torus_mesh()
    v = np.concatenate([v, [[9.0, 9.0, 9.0]]])                            # one vertex no triangle names
    V, T = len(v), len(t)
    assert T == 1200 and T > 1024, "more than one scan tile"
    rng = np.random.default_rng(5)
    dv, dt = _dev(v), _dev(t)
    attrs = {"id": torch.arange(V, device=device()), "xyz32": dv.float()}
    for tag, keep in (("random", rng.uniform(size=T) < 0.4), ("sparse", rng.uniform(size=T) < 0.01), ("all", np.ones(T, dtype=bool)),
                      ("none", np.zeros(T, dtype=bool))):
        want = F.compact_triangles(v, t, keep)
        got = R.compact_triangles(dv, dt, _dev(keep), attrs)
        _assert_compaction(got, want, tag)
        assert got["info"] == {"n_vertices": (V, len(want[0])), "n_triangles": (T, len(want[1]))}
        assert np.array_equal(_np(got["attributes"]["id"]), want[2]) and torch.equal(got["attributes"]["xyz32"], got["vertices"].float())
        _assert_compaction(R.compact_triangles(dv, dt, _dev(keep.astype(np.uint8) * 7)), want, tag + " uint8")
    got = R.compact_triangles(dv, dt, _dev(np.ones(T, dtype=bool)))
    assert np.array_equal(_np(got["vertices"]), v[:-1]) and np.array_equal(_np(got["triangles"]), t), "all kept: only the loose vertex goes"
    got = R.compact_triangles(dv, dt, _dev(np.zeros(T, dtype=bool)))
    assert got["vertices"].shape == (0, 3) and got["triangles"].shape == (0, 3) and got["vertex_index"].shape == (0,)


def test_compact_triangles_drops_a_kept_triangle_with_an_index_out_of_range(R):
    v = np.arange(30, dtype=np.float64).reshape(10, 3)
    t = np.array([[0, 1, 2], [2, 3, 10], [4, 5, 6], [-1, 5, 6], [7, 8, 2 ** 31 - 1], [6, 7, 8], [-2 ** 31, 0, 1], [9, 9, 9]], dtype=np.int32)
    keep = np.array([1, 1, 0, 1, 1, 1, 1, 1], dtype=bool)
    want = F.compact_triangles(v, t, keep)
    assert want[3].tolist() == [0, 5, 7] and want[2].tolist() == [0, 1, 2, 6, 7, 8, 9]
    _assert_compaction(R.compact_triangles(_dev(v), _dev(t), _dev(keep)), want, "bad indices")
    empty = R.compact_triangles(_dev(np.zeros((0, 3))), _dev(np.zeros((0, 3), dtype=np.int32)), _dev(np.zeros(0, dtype=bool)))
    assert empty["vertices"].shape == (0, 3) and empty["triangle_index"].shape == (0,)
    loose = R.compact_triangles(_dev(v), _dev(np.zeros((0, 3), dtype=np.int32)), _dev(np.zeros(0, dtype=bool)))
    assert loose["vertices"].shape == (0, 3) and loose["info"]["n_vertices"] == (10, 0)


# ----------------------------------------------------------------------------------------------------------------- cull_mesh
def _assert_culled(got, want, tag):
    _assert_compaction(got, want[:4], tag)
    assert np.array_equal(_np(got["info"]["votes"]), want[4]), tag
    assert got["info"]["n_vertices"] == (816, len(want[0])) and got["info"]["n_triangles"] == (1620, len(want[1])), tag


def test_cull_mesh_on_the_scene(R):
    s, d = _scene(R)
    v, t = s["vertices"], s["triangles"]
    cams = dict(projections=d["projections"], eyes=d["eyes"])
    ref = lambda masks=s["masks"], **kw: F.cull(v, t, s["projections"], s["eyes"], masks, s["size"], **kw)   # noqa: E731
    # the defaults return exactly the outer sphere, bit for bit
    got = R.cull_mesh(d["vertices"], d["triangles"], masks=d["masks255"], **cams)
    assert np.array_equal(_np(got["vertices"]).view(np.uint64), v[:OUTER_V].view(np.uint64))
    assert np.array_equal(_np(got["triangles"]), t[:OUTER_T])
    assert np.array_equal(_np(got["vertex_index"]), np.arange(OUTER_V)) and np.array_equal(_np(got["triangle_index"]), np.arange(OUTER_T))
    _assert_culled(got, ref(), "defaults")
    info = got["info"]
    assert (info["max_outside"], info["min_seen"], info["occlusion"], info["rule"], info["n_cameras"]) == (0, 1, True, "all", 6)
    assert np.array_equal(_np(info["keep_vertices"]), np.arange(816) < OUTER_V)
    # without occlusion: outer plus inner
    got = R.cull_mesh(d["vertices"], d["triangles"], masks=d["masks255"], occlusion=False, index=d["index"], **cams)
    assert np.array_equal(_np(got["vertices"]), v[:OUTER_V + INNER_V]) and np.array_equal(_np(got["triangles"]), t[:OUTER_T + INNER_T])
    _assert_culled(got, ref(occlusion=False), "no occlusion")
    # without masks: outer plus the floater vertices some camera sees
    got = R.cull_mesh(d["vertices"], d["triangles"], image_size=(48, 48), **cams)
    want = ref(masks=None)
    keep = np.concatenate([np.arange(OUTER_V), 804 + np.flatnonzero(s["counts_nomask"][804:, F.SEEN] >= 1)])
    assert len(keep) > OUTER_V and set(want[2]) <= set(keep) and np.array_equal(want[2][:OUTER_V], np.arange(OUTER_V))
    _assert_culled(got, want, "no masks")
    # rule, thresholds, attributes, masks in another type and with channels
    _assert_culled(R.cull_mesh(d["vertices"], d["triangles"], masks=d["masks255"], rule="any", min_seen=3, **cams), ref(rule="any", min_seen=3), "any")
    assert 0 < ref(rule="all", min_seen=3)[1].shape[0] < ref(rule="any", min_seen=3)[1].shape[0] < OUTER_T
    for min_seen in (1, 0):
        got = R.cull_mesh(d["vertices"], d["triangles"], masks=d["masks255"], max_outside=2, min_seen=min_seen, **cams)
        want = ref(max_outside=2, min_seen=min_seen)
        _assert_culled(got, want, f"max_outside=2 min_seen={min_seen}")
        floater = int((want[2] >= 804).sum())                      # the floater comes back once min_seen allows it
        assert floater == 12 if min_seen == 0 else 0 < floater <= int((s["counts"][804:, F.SEEN] >= 1).sum())
    ids = torch.arange(816, device=device())
    f32 = (d["masks"].float() * 0.75)[..., None].expand(-1, -1, -1, 3).contiguous()
    got = R.cull_mesh(d["vertices"], d["triangles"], masks=f32, attributes={"id": ids}, **cams)
    _assert_culled(got, ref(), "float masks with channels")
    assert torch.equal(got["attributes"]["id"], got["vertex_index"])
    # a dilated mask is another mask: the reference votes on the grown one
    got = R.cull_mesh(d["vertices"], d["triangles"], masks=d["masks255"], dilate=1, **cams)
    grown = _np(R.binary_masks(d["masks255"], dilate=1))
    assert grown.sum() > s["masks"].sum()
    _assert_culled(got, F.cull(v, t, s["projections"], s["eyes"], grown, s["size"]), "dilate=1")


def test_cull_mesh_takes_its_cameras_from_device_rays(R):
    s, d = _scene(R)
    v, t = s["vertices"], s["triangles"]
    maps = np.zeros((6, 48, 48, 3), dtype=np.uint8)
    rays = R.DeviceRays.from_source_maps(maps, maps, s["masks"] * np.uint8(255), torch.from_numpy(s["intrinsics_inv"]),
                                         torch.from_numpy(s["pose"]), "cuda:0")
    # the cameras as DeviceRays holds them (float32), through the same host arithmetic
    P32, eyes32 = R.camera_projections(rays.intrinsics_all_inv, rays.pose_all)
    want = F.cull(v, t, P32.numpy(), eyes32.numpy(), s["masks"], s["size"])
    got = R.cull_mesh(d["vertices"], d["triangles"], rays=rays)
    _assert_culled(got, want, "DeviceRays")
    assert np.array_equal(want[4], s["counts"]), "float32 cameras of this scene give the votes of the float64 ones"
    sub = [0, 2, 4]
    want = F.cull(v, t, P32.numpy()[sub], eyes32.numpy()[sub], s["masks"][sub], s["size"])
    got = R.cull_mesh(d["vertices"], d["triangles"], rays=rays, views=sub)
    _assert_culled(got, want, "views=[0, 2, 4]")
    assert got["info"]["n_cameras"] == 3 and bool((got["info"]["votes"].sum(dim=1) == 3).all())
    with pytest.raises(IndexError, match="out of range"):
        R.cull_mesh(d["vertices"], d["triangles"], rays=rays, views=[6])


# ------------------------------------------------------------------------------------------------------------- the renderer
def _tiny_renderer(R):
    from rnb_neus_fork_amd import checkpoint as CK
    dev = device()
    z = np.load(os.path.join(GOLDEN, "ref_ckpt_tiny_step3.npz"), allow_pickle=False)
    nc = z["nerf.conf"]
    torch.manual_seed(99)
    nerf = R.NeRF(D=int(nc[0]), W=int(nc[1]), d_in=int(nc[2]), d_in_view=int(nc[3]), multires=int(nc[4]),
                  multires_view=int(nc[5]), output_ch=int(nc[6]), skips=[int(nc[7])], use_viewdirs=True).to(dev)
    sdf = R.SDFNetwork(d_in=3, d_out=65, d_hidden=64, n_layers=8, skip_in=[4], multires=6).to(dev)
    devn = R.SingleVarianceNetwork(0.1).to(dev)
    col = R.RenderingNetwork(d_feature=64, mode="no_view_dir", d_in=6, d_out=3, d_hidden=64, n_layers=2, multires_view=4).to(dev)
    ren = R.NeuSRenderer(nerf, sdf, devn, col, n_samples=16, n_importance=16, n_outside=0, up_sample_steps=4, perturb=1.0)
    params = list(nerf.parameters()) + list(sdf.parameters()) + list(devn.parameters()) + list(col.parameters())
    CK.load_checkpoint(os.path.join(GOLDEN, "ref_ckpt_tiny.pth"), nerf, sdf, devn, col, R.FlatAdam(params, lr=1.0), map_location=dev)
    return ren


def test_the_renderer_cull_keyword(R):
    from tests.mesh_attrs_util import HI, LO
    s, d = _scene(R)
    ren = _tiny_renderer(R)
    res = 40
    plain_v, plain_t = ren.extract_geometry(LO, HI, res, threshold=0.0, backend="native")
    assert ren.last_mesh_cull is None and len(plain_t) > 500
    # three of the scene's cameras, each with the left half of its mask cut away: what only they would support goes
    masks = s["masks"][:3].copy()
    masks[:, :, :24] = 0
    cull = dict(projections=d["projections"][:3], eyes=d["eyes"][:3], masks=_dev(masks * np.uint8(255)), max_outside=1)
    want = R.cull_mesh(_dev(plain_v), _dev(plain_t.astype(np.int32)), **cull)
    assert 0 < want["triangles"].shape[0] < len(plain_t), "the cameras of this test must remove something and keep something"
    cv, ct = ren.extract_geometry(LO, HI, res, threshold=0.0, backend="native", cull=cull)
    assert cv.dtype == np.float64 and np.array_equal(ct, _np(want["triangles"])) and np.array_equal(cv, _np(want["vertices"]))
    assert np.array_equal(cv, plain_v[_np(want["vertex_index"])])
    info = ren.last_mesh_cull
    assert info["n_triangles"] == (len(plain_t), len(ct)) and np.array_equal(_np(info["votes"]), _np(want["info"]["votes"]))
    # after the cleaning, before the simplification
    kv, kt = ren.extract_geometry(LO, HI, res, threshold=0.0, backend="native", clean={"keep_largest": 1}, cull=cull,
                                  simplify=dict(cell_size=2.0))
    assert ren.last_mesh_clean["n_triangles"][1] == ren.last_mesh_cull["n_triangles"][0]
    assert ren.last_mesh_cull["n_triangles"][1] == ren.last_mesh_simplify["n_triangles"][0] and 0 < len(kt) < len(ct)
    # the textured path: attributes of the surviving vertices alone
    tex = ren.extract_textured_geometry(LO, HI, res, cull=cull)
    assert np.array_equal(tex["triangles"], ct) and np.array_equal(tex["vertices"], cv) and len(tex["normals"]) == len(cv)
    gv = R.marching_cubes(ren.extract_fields(LO, HI, res, to_host=False), 0.0)[0]
    direct = ren.vertex_attributes(grid_vertices=gv.index_select(0, want["vertex_index"]), bounds=(LO, HI), resolution=res)
    for k_tex, k_at in (("normals", "normal"), ("sdf", "sdf"), ("albedo", "albedo"), ("colors", "rgb")):
        assert np.array_equal(tex[k_tex], _np(direct[k_at])), k_tex
    full = ren.extract_textured_geometry(LO, HI, res)
    # cull=None: bit-identical to the call without the keyword
    nv, nt = ren.extract_geometry(LO, HI, res, threshold=0.0, backend="native", cull=None)
    assert np.array_equal(nv.view(np.uint64), plain_v.view(np.uint64)) and np.array_equal(nt, plain_t)
    none = ren.extract_textured_geometry(LO, HI, res, cull=None)
    assert all(np.array_equal(none[k], full[k]) for k in full) and sorted(none) == sorted(full)
    with pytest.raises(ValueError, match="rule"):
        ren.extract_geometry(LO, HI, res, backend="native", cull=dict(cull, rule="most"))
