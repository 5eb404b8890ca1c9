"""The mesh tools past 2^20 items: every loop that takes a second trip only at that size, on the meshes and camera sets of
tests/mesh_large_shapes.py (whose analytic answers tests/test_mesh_large_shapes_host.py checks on the host).

  scan_block_sums_kernel<unsigned> (csrc/scan.hip.h), two arrays of different length: compaction by a per-triangle keep,
      compaction by component, simplification — T in two chunks and V in one (SHEET), V in two and T in one (PREFIX)
  the same kernel on one array: the root-rank scan of the components — V in four chunks (ISOLATED)
  me_area_blocks_kernel (csrc/mesh_eval.hip): the fp64 chain over the tile sums, `carry` across chunks (ISOLATED)
  cv_kernel (csrc/mesh_cull.hip): the workgroup loop with the stride of a grid capped at 2^20

Each test asserts the tile, chunk or workgroup count that makes its loop take the trip before it calls the device, so a
change of kScanTile, of the chunk width or of kCvMaxBlocks fails the test instead of un-testing the loop.  Every integer
output and every copied coordinate is compared for equality (coordinates as uint64 bits); the two floating-point sums are
held to derived bounds: `mesh_components_ref.area_bound` per component, (T + 8) 2^-52 A for the area scan."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import mesh_components_ref as MC
from tests import mesh_cull_ref as CU
from tests import mesh_distance_ref as MD
from tests import mesh_large_shapes as L
from tests import mesh_simplify_ref as MS
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device

pytestmark = pytest.mark.gpu

LINE = L.LINE
_ON_DEVICE = {}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device())


def _np(x):
    return x.detach().cpu().numpy()


def _mesh(name):
    """(the instance, its vertices and triangles on the device), uploaded once"""
    d = L.big(name)
    if name not in _ON_DEVICE:
        _ON_DEVICE[name] = (_dev(d["vertices"]), _dev(d["triangles"]))
    return (d,) + _ON_DEVICE[name]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _two_array_trips(name):
    """the tile arithmetic of the two-array instance: exactly one of V and T is past 2^20"""
    d = L.big(name)
    V, T = len(d["vertices"]), len(d["triangles"])
    nbv, nbt = L.tiles(V), L.tiles(T)
    if name == "SHEET":
        assert nbv <= L.CHUNK < nbt <= 2 * L.CHUNK, f"SHEET: {nbv} / {nbt} tiles: n0 fits one chunk, n1 needs two"
    else:
        assert nbt <= L.CHUNK < nbv <= 2 * L.CHUNK, f"PREFIX: {nbv} / {nbt} tiles: n0 needs two chunks, n1 fits one"
    return V, T


# ---------------------------------------------------------------------------------------- a. compaction by a per-triangle keep
def _keep(name, tag):
    d = L.big(name)
    t = d["triangles"]
    T = len(t)
    if tag == "random":
        return L.random_keep(T)
    if tag == "all":
        return np.ones(T, dtype=bool)
    keep = np.zeros(T, dtype=bool)
    if tag == "tail_only":                    # triangle 0 plus every triangle >= 2^20 - 3 (on PREFIX: triangle 0 alone)
        keep[0] = True
        keep[LINE - 3:] = True
    elif tag == "tail_vertices":              # triangle 0 plus every triangle that names a vertex >= 2^20 - 3
        keep[0] = True
        keep |= (t >= LINE - 3).any(axis=1)
    else:
        assert tag == "last_row" and name == "PREFIX"
        keep[-2 * 500:] = True                # nothing but the sheet's last row of quads
    return keep


@pytest.mark.parametrize("name,tag", [("SHEET", "random"), ("SHEET", "tail_only"), ("SHEET", "all"), ("PREFIX", "random"),
                                      ("PREFIX", "tail_only"), ("PREFIX", "tail_vertices"), ("PREFIX", "all"), ("PREFIX", "last_row")])
def test_compact_triangles_past_the_first_chunk(R, name, tag):
    """rnb_mesh_compact_triangles_count / _emit: scan_block_sums_kernel<unsigned> with narr = 2 and n0 != n1.  On SHEET the
    triangle tile sums (1,027) take the second trip of the chunk loop and the vertex tile sums (515) do not; on PREFIX it is
    the other way round (1,027 / 489).  From the second chunk on carry_s decides where every kept triangle (SHEET) or vertex
    (PREFIX) lands; with "tail_only" / "tail_vertices" nearly everything kept lies past 2^20, so nearly every position is
    carry plus a few."""
    V, T = _two_array_trips(name)
    d, dv, dt = _mesh(name)
    keep = _keep(name, tag)
    want = CU.compact_triangles(d["vertices"], d["triangles"], keep)
    v, t, vi, ti = want
    past = int((ti >= LINE).sum()) if name == "SHEET" else int((vi >= LINE).sum())
    print(f"{name} {tag}: {len(ti)} of {T} triangles, {len(vi)} of {V} vertices kept; {past} past 2^20")
    if not (name == "PREFIX" and tag == "tail_only"):
        assert past > 300, "the fixture moved: nothing kept past 2^20"
    if tag in ("tail_only", "tail_vertices") and name == "SHEET":
        assert len(ti) == 1 + 3 + (T - LINE) and ti[0] == 0 and ti[1] == LINE - 3, "the fixture moved"
    got = R.compact_triangles(dv, dt, _dev(keep))
    assert got["info"] == {"n_vertices": (V, len(vi)), "n_triangles": (T, len(ti))}, f"{name} {tag}: the totals of the scan"
    assert got["vertices"].dtype == torch.float64 and got["triangles"].dtype == torch.int32
    assert got["vertex_index"].dtype == torch.int64 and got["triangle_index"].dtype == torch.int64
    assert np.array_equal(_np(got["triangle_index"]), ti), f"{name} {tag}: triangle_index"
    assert np.array_equal(_np(got["vertex_index"]), vi), f"{name} {tag}: vertex_index"
    assert _np(got["triangles"]).shape == t.shape and np.array_equal(_np(got["triangles"]), t), f"{name} {tag}: triangles"
    assert _np(got["vertices"]).shape == v.shape and np.array_equal(_bits(_np(got["vertices"])), _bits(v)), f"{name} {tag}: vertices"


# ------------------------------------------------------------------------------------------- b. components and cleaning
def test_components_and_cleaning_of_the_sheet(R):
    """rnb_mesh_compact_count / _emit on SHEET: the two-array block-sum scan with 515 vertex tiles (one trip) and 1,027
    triangle tiles (two trips).  keep_largest=1 drops triangle 0 and the last one, so every triangle past 2^20 lands at its
    own index minus one: the carry of the second chunk.  The labels are analytic (floater, sheet, floater)."""
    V, T = _two_array_trips("SHEET")
    d, dv, dt = _mesh("SHEET")
    v, t, labels = d["vertices"], d["triangles"], d["labels"]
    got = R.mesh_components(dt, vertices=dv)
    assert got["n_components"] == 3
    assert np.array_equal(_np(got["labels"]), labels), "labels"
    assert _np(got["triangles"]).tolist() == [1, T - 2, 1] and _np(got["vertices"]).tolist() == [3, V - 6, 3]
    parts = (slice(0, 3), slice(3, V - 3), slice(V - 3, V))
    assert np.array_equal(_np(got["bbox_min"]), np.stack([v[p].min(axis=0) for p in parts]))
    assert np.array_equal(_np(got["bbox_max"]), np.stack([v[p].max(axis=0) for p in parts]))
    area = np.bincount(labels[t[:, 0]], weights=MC.triangle_areas(v, t), minlength=3)
    bound = MC.area_bound(v, t, labels, 3)
    err = np.abs(_np(got["area"]) - area)
    print(f"SHEET: area |dev - ref| = {err / bound} of (n_c + 16) 2^-52 S_c")
    assert (err <= bound).all(), f"area off by {(err / bound).max():.2f} of the bound"
    out = R.clean_mesh(dv, dt, keep_largest=1)
    assert out["info"]["n_components"] == 3 and _np(out["info"]["kept"]).tolist() == [1]
    assert out["info"]["n_vertices"] == (V, V - 6) and out["info"]["n_triangles"] == (T, T - 2)
    assert np.array_equal(_np(out["vertex_index"]), np.arange(3, V - 3))
    assert np.array_equal(_np(out["triangles"]), t[1:-1] - 3), "the sheet alone, indices shifted by 3"
    assert np.array_equal(_bits(_np(out["vertices"])), _bits(v[3:-3]))


def test_cleaning_drops_the_unreferenced_prefix(R):
    """rnb_mesh_components (one array, 1,027 vertex tiles: the root-rank scan's second trip, with its only set flag at
    vertex 800,000) and rnb_mesh_compact_count / _emit with n0 = 1,027 > 1,024 > n1 = 489: the mirror of SHEET.  No
    criterion: only the 800,000 vertices no triangle names go, and the sheet comes back bit for bit; 2,425 of its vertices
    have an index >= 2^20 and take their position from the carry."""
    V, T = _two_array_trips("PREFIX")
    d, dv, dt = _mesh("PREFIX")
    v, t, n_loose = d["vertices"], d["triangles"], d["n_loose"]
    out = R.clean_mesh(dv, dt)
    assert out["info"]["n_components"] == 1 and out["info"]["n_vertices"] == (V, V - n_loose) and out["info"]["n_triangles"] == (T, T)
    assert np.array_equal(_np(out["vertex_index"]), np.arange(n_loose, V))
    assert np.array_equal(_np(out["triangles"]), t - n_loose)
    assert np.array_equal(_bits(_np(out["vertices"])), _bits(v[n_loose:]))
    labels = _np(R.mesh_components(dt, n_vertices=V)["labels"])
    assert (labels[:n_loose] == -1).all() and (labels[n_loose:] == 0).all()


def test_a_million_components(R):
    """rnb_mesh_components on ISOLATED: scan_block_sums_kernel<unsigned> with narr = 1 over 3,085 vertex tiles, four trips,
    the carry handed on three times; every third vertex is a root, so the rank of root 3 j is j and any lost carry shows
    in every label past it.  Then clean_mesh(by="area", min_fraction=0.01): the two-array scan with four and two trips."""
    d, dv, dt = _mesh("ISOLATED")
    v, t, labels, areas = d["vertices"], d["triangles"], d["labels"], d["areas"]
    V, T = len(v), len(t)
    assert L.tiles(V) == 3085 and L.chunks(V) == 4 and L.chunks(T) == 2, "four trips over the vertex tiles, two over the triangles'"
    got = R.mesh_components(dt, vertices=dv)
    assert got["n_components"] == T
    assert np.array_equal(_np(got["labels"]), labels), "labels[v] = v // 3"
    assert bool((got["triangles"] == 1).all()) and bool((got["vertices"] == 3).all()) and got["triangles"].shape == (T,)
    corners = v.reshape(T, 3, 3)
    assert np.array_equal(_np(got["bbox_min"]), corners.min(axis=1)) and np.array_equal(_np(got["bbox_max"]), corners.max(axis=1))
    bound = MC.area_bound(v, t, labels, T)
    err = np.abs(_np(got["area"]) - areas)
    print(f"ISOLATED: area |dev - ref| at most {float((err / bound).max()):.3f} of (n_c + 16) 2^-52 S_c")
    assert (err <= bound).all()
    out = R.clean_mesh(dv, dt, by="area", min_fraction=0.01)
    measure = _np(out["info"]["measure"])
    assert np.array_equal(measure, _np(got["area"])), "two runs of the statistics give the same bits"
    # the keep from the device's own measure: a one-ulp tie at the threshold cannot fail the test
    keep = MC.select(measure, np.ones(T, dtype=np.int64), min_fraction=0.01)
    n_kept = int(keep.sum())
    past = int(keep[LINE:].sum())
    print(f"ISOLATED min_fraction=0.01: {n_kept} of {T} components kept, {past} of them past 2^20")
    assert 0.2 * T < n_kept < 0.9 * T and past > 500, "the fixture moved"
    v1, t1, index = MC.compact(v, t, labels, keep)
    assert out["info"]["n_vertices"] == (V, len(v1)) and out["info"]["n_triangles"] == (T, len(t1))
    assert np.array_equal(_np(out["info"]["kept"]), np.flatnonzero(keep))
    assert np.array_equal(_np(out["vertex_index"]), index) and np.array_equal(_np(out["triangles"]), t1)
    assert np.array_equal(_bits(_np(out["vertices"])), _bits(v1))


# ----------------------------------------------------------------------------------------------------- c. simplification
SIMPLIFY_CELL = 0.03        # 2.3 x 2.7 grid spacings of the sheet: about one triangle in six survives


@pytest.mark.parametrize("name", ["SHEET", "PREFIX"])
def test_simplification_past_the_first_chunk(R, name):
    """rnb_mesh_simplify_count / _emit: scan_block_sums_kernel<unsigned> with narr = 2 over the flags "vertex is the leader
    of a surviving cluster" and "triangle survives".  SHEET: 1,027 triangle tiles, the survivors past triangle 2^20 land
    where the carry of the second chunk says; PREFIX: 1,027 vertex tiles, the same for the leaders past vertex 2^20."""
    V, T = _two_array_trips(name)
    d, dv, dt = _mesh(name)
    want = MS.simplify(d["vertices"], d["triangles"], SIMPLIFY_CELL)
    share = want["counts"][1] / T
    spread = want["triangle_index"] if name == "SHEET" else want["vertex_index"]
    past = int((spread >= LINE).sum())
    print(f"{name} h = {SIMPLIFY_CELL}: {want['counts']}, {share:.1%} of the triangles survive, {past} survivors past 2^20")
    before = int((spread < LINE).sum())
    assert 0.10 <= share <= 0.20 and past > 100 and before > 10000, "the fixture moved: the survivors lie on both sides of 2^20"
    out = R.simplify_mesh(dv, dt, cell_size=SIMPLIFY_CELL)
    info = out["info"]
    got = {k: _np(out[k]) for k in ("vertices", "triangles", "vertex_index", "vertex_cluster", "triangle_index")}
    got["counts"] = [info["n_vertices"][1], info["n_triangles"][1], info["n_degenerate"], info["n_duplicate"],
                     int(info["skipped"]["bad_index"]) | 2 * int(info["skipped"]["bad_vertex"]), info["n_clusters"]]
    assert got["counts"] == want["counts"], f"{name}: counts {got['counts']}, reference {want['counts']}"
    assert np.array_equal(_np(info["origin"]), want["origin"])
    for k in ("triangle_index", "vertex_index", "vertex_cluster", "triangles"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), f"{name}: {k}"
    assert np.array_equal(_bits(got["vertices"]), _bits(want["vertices"])), f"{name}: vertices"
    assert MS.equal(got, want)


# ------------------------------------------------------------------------------------------ d. the area scan and the samples
def _area_scan(R, dv, dt):
    """rnb_mesh_sample_areas with the sizing of mesh_eval.sample_surface: (cum [T], total) as numpy"""
    lib, nat = R.native.load(), R.native
    V, T = dv.shape[0], dt.shape[0]
    nbytes = C.c_int64()
    nat.check(lib.rnb_mesh_sample_workspace_bytes(T, C.byref(nbytes)))
    assert nbytes.value >= 8 * L.tiles(T), "one fp64 sum per tile"
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dv.device)
    cum = torch.empty(T, dtype=torch.float64, device=dv.device)
    head = torch.empty(2, dtype=torch.float64, device=dv.device)
    with nat.on_device(dv.device) as stream:
        nat.check(lib.rnb_mesh_sample_areas(nat.ptr(dv), V, nat.ptr(dt), T, nat.ptr(ws), ws.numel(), nat.ptr(cum), nat.ptr(head),
                                            stream))
    return _np(cum), _np(head[:1])


def test_the_area_scan_past_the_first_chunk(R):
    """me_area_blocks_kernel on ISOLATED: 1,029 tile sums, so the serial fp64 chain goes through a second chunk (of 5 tiles)
    that starts from `carry`.  |cum - np.cumsum(areas)| <= (T + 8) 2^-52 A everywhere: two summation orders of T
    non-negative terms each lie within (T - 1) 2^-53 A of the exact sum, the 8 covers a few ulps of area evaluation per
    triangle.  A carry dropped at the second chunk misses this bound by a factor 4 x 10^9 at every one of the 4,101
    triangles past 2^20, the honest order meets it with a factor 3,600 to spare (tests/test_mesh_large_shapes_host.py)."""
    d, dv, dt = _mesh("ISOLATED")
    areas = d["areas"]
    T = len(areas)
    assert L.tiles(T) == 1029 and L.chunks(T) == 2 and T - LINE == 4101, "the chain over the tile sums takes a second trip"
    cum, total = _area_scan(R, dv, dt)
    assert (np.diff(cum) >= 0.0).all(), "cum is non-decreasing"
    assert cum[-1:].view(np.uint64) == total.view(np.uint64), "cum[T - 1] has the bits of the total"
    bound = L.area_scan_bound(areas)
    err = np.abs(cum - np.cumsum(areas))
    print(f"area scan, T = {T}: |cum - cumsum| at most {float(err.max()) / bound:.2e} of (T + 8) 2^-52 A, "
          f"{float(err[LINE:].max()) / bound:.2e} past 2^20")
    assert (err <= bound).all(), f"the area scan is {float(err.max()) / bound:.3e} of its bound off, first at triangle {int(np.argmax(err > bound))}"


def test_surface_samples_past_the_first_chunk(R):
    """sample_surface on ISOLATED with 2,100,000 samples (two per triangle on average): the samples find their triangle
    by bisection in the scanned areas, so the 0.40 % of the area past triangle 2^20 must receive its 8,300 samples."""
    d, dv, dt = _mesh("ISOLATED")
    v, t, area = d["vertices"], d["triangles"], d["areas"]
    T, n = len(t), 2_100_000
    assert L.chunks(T) == 2
    out = R.sample_surface(dv, dt, n, seed=3)
    pts, tri, bary, nrm = (_np(out[k]) for k in ("points", "triangle", "bary", "normal"))
    assert pts.shape == (n, 3) and tri.shape == (n,) and tri.dtype == np.int32 and bary.shape == (n, 3) and nrm.shape == (n, 3)
    assert abs(out["area"] - area.sum()) <= 1e-12 * area.sum()
    assert tri.min() >= 0 and tri.max() < T
    assert (bary >= 0).all() and np.abs((bary[:, 0] + bary[:, 1]) + bary[:, 2] - 1.0).max() <= 4 * MD.EPS
    for k in (0, 1, 2, 77, n - 1):
        assert tuple(bary[k]) == MD.sample_bary(3, k), f"sample {k}: the weights are not those of the documented mixer"
    corners = v[t[tri]]
    want = (bary[:, 0, None] * corners[:, 0] + bary[:, 1, None] * corners[:, 1]) + bary[:, 2, None] * corners[:, 2]
    scale = np.abs(corners).max(axis=(1, 2))
    assert (np.abs(pts - want).max(axis=1) <= 4 * MD.EPS * scale).all()
    ln = np.sqrt((nrm * nrm).sum(axis=1))
    assert np.abs(ln - 1.0).max() <= 4 * MD.EPS
    e1, e2 = corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]
    assert (np.abs((nrm * e1).sum(1)) <= 1e-12 * np.sqrt((e1 * e1).sum(1))).all() and ((nrm * np.cross(e1, e2)).sum(1) > 0).all()
    counts = np.bincount(tri, minlength=T)
    expected = n * area / area.sum()
    dev_ = np.abs(counts - expected)
    past = int(counts[LINE:].sum())
    print(f"surface samples: worst |c_t - n A_t / A| = {dev_.max():.3f} (past 2^20: {dev_[LINE:].max():.3f}); {past} samples past "
          f"triangle 2^20, {expected[LINE:].sum():.0f} expected")
    assert dev_.max() <= 2.0
    assert (counts[expected >= 3.0] > 0).all(), "a triangle that expects three samples or more received none"
    assert 7000 < expected[LINE:].sum() < 10000, "the fixture moved"
    assert past > 4000


# ------------------------------------------------------------------------------------------------------------- e. the votes
def _vote_index(R):
    return R.MeshIndex(_dev(L.TWO_TRIANGLES_V), _dev(L.TWO_TRIANGLES_T))


def test_votes_of_more_cameras_than_the_grid_holds_workgroups(R):
    """cv_kernel with N = 5 points and C = 2^20 + 261 cameras: nbp = 1, so workgroup b is camera b, the grid is capped at
    2^20 workgroups and the cameras >= 2^20 are the second trips (b += gridDim.x) of workgroups 0 .. 260.  Every eye is the
    origin: SEEN / OCCLUDED of a pair that reaches the cast is that point's answer from one camera of the reference.  The
    whole status [C, 5] and the counts are compared with the reference bit for bit, with and without occlusion."""
    pts, size = L.VOTE_POINTS, (16, 16)
    N, n_cam = len(pts), 2 ** 20 + 261
    nbp = (N + L.CV_THREADS - 1) // L.CV_THREADS
    total = nbp * n_cam
    assert nbp == 1 and L.CV_MAX_BLOCKS < total < 2 * L.CV_MAX_BLOCKS and total - L.CV_MAX_BLOCKS == 261, \
        "workgroups 0 .. 260 take a second trip"
    P, masks = L.shifted_cameras(n_cam, seed=1)
    assert masks.nbytes == n_cam * 256
    reaches, base = np.empty((n_cam, N), dtype=bool), np.empty((n_cam, N), dtype=np.uint8)
    for i, p in enumerate(pts):
        reaches[:, i], base[:, i] = L.votes_one_point(p, P, masks, size)[:2]
    cast = L.seen_from_the_origin(pts)
    index = _vote_index(R)
    dp, dP, deyes, dmasks = _dev(pts), _dev(P), torch.zeros(n_cam, 3, dtype=torch.float64, device=device()), _dev(masks)
    for occlusion in (True, False):
        status = np.where(reaches, cast[None, :] if occlusion else CU.SEEN, base).astype(np.uint8)
        counts = np.stack([(status == k).sum(axis=0) for k in range(4)], axis=1).astype(np.int32)
        tail = np.bincount(status[L.CV_MAX_BLOCKS:].reshape(-1), minlength=4)
        print(f"occlusion={occlusion}: statuses among the cameras >= 2^20: {tail.tolist()}; counts {counts.tolist()}")
        assert (tail[[0, 1, 3]] > 0).all() and (tail[2] > 0) == occlusion, "the fixture moved: a status does not occur past 2^20"
        got = index.view_votes(dp, dP, deyes, dmasks, occlusion=occlusion, return_status=True)
        st = _np(got["status"])
        assert st.shape == (n_cam, N) and st.dtype == np.uint8
        wrong = np.flatnonzero((st != status).any(axis=1))
        assert len(wrong) == 0, f"occlusion={occlusion}: status differs for {len(wrong)} cameras, first {wrong[:5]}, {(wrong >= L.CV_MAX_BLOCKS).sum()} of them past 2^20"
        assert np.array_equal(_np(got["counts"]), counts), f"occlusion={occlusion}: counts {_np(got['counts']).tolist()}"


def test_votes_where_the_second_trip_splits_into_camera_and_point_half(R):
    """cv_kernel with N = 257 points (nbp = 2) and C = 2^19 + 3 cameras: total = 2^20 + 6 workgroups, so workgroups 0 .. 5
    take a second trip, where b = 2^20 + j decomposes into the cameras c = 2^19 + j // 2 >= 2^19 and both point halves
    (256 points and 1).  Status is held to the reference on the three cameras >= 2^19 and on 64 sampled others; for ALL
    pairs the kernel's two outputs must agree, counts[:, k] == (status == k).sum(0) — a consistency check of the kernel
    with itself, not with the reference: the sampled comparison is what ties status to the reference."""
    N, n_cam, size = 257, 2 ** 19 + 3, (16, 16)
    nbp = (N + L.CV_THREADS - 1) // L.CV_THREADS
    total = nbp * n_cam
    assert nbp == 2 and total == L.CV_MAX_BLOCKS + 6 and (total - 1) // nbp == n_cam - 1 and L.CV_MAX_BLOCKS // nbp == 2 ** 19, \
        "the second trip covers the cameras >= 2^19 with both point halves"
    pts = L.vote_points(N)
    P, masks = L.shifted_cameras(n_cam, seed=4)
    sample = np.concatenate([np.sort(np.random.default_rng(9).choice(2 ** 19, 64, replace=False)), np.arange(2 ** 19, n_cam)])
    index = _vote_index(R)
    dp, dP, deyes, dmasks = _dev(pts), _dev(P), torch.zeros(n_cam, 3, dtype=torch.float64, device=device()), _dev(masks)
    for occlusion in (True, False):
        want = CU.view_votes(pts, P[sample], np.zeros((len(sample), 3)), masks[sample], size, L.TWO_TRIANGLES_V, L.TWO_TRIANGLES_T,
                             occlusion=occlusion)[0]
        seen_past = np.bincount(want[-3:].reshape(-1), minlength=4)
        assert (seen_past[[0, 1, 3]] > 0).all() and (seen_past[2] > 0) == occlusion, "the fixture moved: a status does not occur past 2^19"
        got = index.view_votes(dp, dP, deyes, dmasks, occlusion=occlusion, return_status=True)
        st = got["status"].index_select(0, _dev(sample))
        assert np.array_equal(_np(st), want), f"occlusion={occlusion}: status of the sampled cameras and those >= 2^19"
        assert np.array_equal(_np(st)[-3:, 256], want[-3:, 256]), "the second point half: one point"
        per_status = torch.stack([(got["status"] == k).sum(dim=0) for k in range(4)], dim=1)
        assert torch.equal(per_status.to(torch.int32), got["counts"]), f"occlusion={occlusion}: counts are not the column sums of status"
        assert bool((got["counts"].sum(dim=1) == n_cam).all())
