"""tests/mesh_large_shapes.py checked on the host: the analytic labels against the sequential union-find on small instances,
the one-point vote reference against the per-camera loop, the sizes and tile counts of the three big instances, and the
proof that the bound of the area scan tells the honest summation order from a scan that loses its carry at the second
chunk.  The integer chunk loop and the vote kernel's workgroup loop are restated in numpy the same way: a lost carry or
a loop of one trip changes exactly the items past 2^20 that the device tests compare.  No device."""
import numpy as np

from tests import mesh_components_ref as MC
from tests import mesh_cull_ref as CU
from tests import mesh_large_shapes as L


def test_analytic_labels_are_the_union_find_labels_on_small_instances():
    for m, k in ((5, 7), (1, 1), (3, 2)):
        v, t, labels = L.sheet_with_floaters(m, k)
        assert len(v) == (m + 1) * (k + 1) + 6 and len(t) == 2 * m * k + 2
        want, n = MC.components(t, len(v))
        assert n == 3 and np.array_equal(labels, want) and labels.dtype == want.dtype
        st = MC.stats(t, want, n)
        assert st["triangles"].tolist() == [1, 2 * m * k, 1] and st["vertices"].tolist() == [3, len(v) - 6, 3]
        # the sheet's own indices are the whole mesh's shifted by 3
        sv, stri = L.sheet(m, k)
        assert np.array_equal(t[1:-1] - 3, stri) and np.array_equal(v[3:-3].view(np.uint64), sv.view(np.uint64))
    for n in (1, 9, 257):
        v, t = MC.isolated(n)
        want, c = MC.components(t, len(v))
        assert c == n and np.array_equal(L.isolated_labels(n), want)
    v, t = L.prefix(11, 5, 7)
    want, c = MC.components(t, len(v))
    assert c == 1 and (want[:11] == -1).all() and (want[11:] == 0).all()
    sv, stri = L.sheet(5, 7)
    assert np.array_equal(t - 11, stri) and np.array_equal(v[11:].view(np.uint64), sv.view(np.uint64)) and np.isfinite(v).all()


def test_the_sheet_is_not_planar_and_its_last_row_ends_the_arrays():
    v, t = L.sheet(5, 7)
    assert np.ptp(v[:, 2]) > 1e-3 and len(np.unique(v, axis=0)) == len(v)
    assert MC.triangle_areas(v, t).min() > 0.0
    last_row = t[-2 * 7:]                                     # the last row of quads: the vertices of the last two rows
    assert last_row.min() == 4 * 8 and last_row.max() == len(v) - 1


def _votes_by_point(points, P, masks, size):
    status = np.empty((len(P), len(points)), dtype=np.uint8)
    for i, p in enumerate(points):
        reaches, st, _, _ = L.votes_one_point(p, P, masks, size)
        st[reaches] = CU.SEEN
        status[:, i] = st
    return status


def test_votes_one_point_is_the_per_camera_loop():
    s = CU.scene()
    no_v, no_t = np.zeros((3, 3)), np.zeros((0, 3), dtype=np.int32)
    want = CU.view_votes(s["vertices"], s["projections"], s["eyes"], s["masks"], s["size"], no_v, no_t, occlusion=False)[0]
    assert np.array_equal(_votes_by_point(s["vertices"], s["projections"], s["masks"], s["size"]), want)
    assert len(np.unique(want)) == 3, "out of frame, outside the mask and seen all occur on the scene"
    # 1,000 shifted cameras with random masks on the five points of the vote tests (one NaN, one behind the cameras)
    P, masks = L.shifted_cameras(1000, seed=2)
    want = CU.view_votes(L.VOTE_POINTS, P, np.zeros((1000, 3)), masks, (16, 16), no_v, no_t, occlusion=False)[0]
    got = _votes_by_point(L.VOTE_POINTS, P, masks, (16, 16))
    assert np.array_equal(got, want)
    assert (want[:, 3:] == CU.OUT_OF_FRAME).all() and {CU.OUT_OF_FRAME, CU.OUTSIDE_MASK, CU.SEEN} == set(np.unique(want[:, :3]))
    # without masks
    want = CU.view_votes(L.VOTE_POINTS, P, np.zeros((1000, 3)), None, (16, 16), no_v, no_t, occlusion=False)[0]
    assert np.array_equal(_votes_by_point(L.VOTE_POINTS, P, None, (16, 16)), want)
    # the one-camera answer of the cast: the three points of the two-triangle test, nothing cast for the other two
    assert L.seen_from_the_origin(L.VOTE_POINTS).tolist() == [CU.OCCLUDED, CU.SEEN, CU.SEEN, CU.OUT_OF_FRAME, CU.OUT_OF_FRAME]
    pts = L.vote_points(257)
    st = L.seen_from_the_origin(pts)
    assert len(pts) == 257 and (st == CU.SEEN).sum() > 30 and (st == CU.OCCLUDED).sum() > 30 and (st == CU.OUT_OF_FRAME).sum() >= 16


def test_sizes_and_tile_counts_of_the_big_instances():
    """`big` asserts them itself ("the fixture moved"); here they are stated once more against the table of the tests"""
    s, p, i = L.big("SHEET"), L.big("PREFIX"), L.big("ISOLATED")
    sizes = {k: (len(d["vertices"]), len(d["triangles"])) for k, d in (("SHEET", s), ("PREFIX", p), ("ISOLATED", i))}
    assert sizes == {"SHEET": (527082, 1051252), "PREFIX": (1051001, 500000), "ISOLATED": (3158031, 1052677)}
    assert {k: (L.tiles(v), L.tiles(t)) for k, (v, t) in sizes.items()} == \
        {"SHEET": (515, 1027), "PREFIX": (1027, 489), "ISOLATED": (3085, 1029)}
    assert {k: (L.chunks(v), L.chunks(t)) for k, (v, t) in sizes.items()} == {"SHEET": (1, 2), "PREFIX": (2, 1), "ISOLATED": (4, 2)}
    assert L.LINE == 2 ** 20 and L.tiles(L.LINE) == 1024 and L.chunks(L.LINE) == 1 and L.chunks(L.LINE + 1) == 2
    # without the floaters
    assert (726 * 726, 2 * 725 * 725) == (527076, 1051250) and (L.tiles(527076), L.tiles(1051250)) == (515, 1027)
    # what lies past the line
    assert int((np.arange(len(s["triangles"])) >= L.LINE).sum()) == 2676
    referenced = np.zeros(len(p["vertices"]), dtype=bool)
    referenced[p["triangles"].reshape(-1)] = True
    assert int(referenced[L.LINE:].sum()) == 2425 and not referenced[:p["n_loose"]].any() and referenced[p["n_loose"]:].all()
    assert len(i["triangles"]) - L.LINE == 4101 and np.array_equal(i["labels"], np.arange(len(i["vertices"])) // 3)
    assert s["labels"][:3].tolist() == [0, 0, 0] and s["labels"][-3:].tolist() == [2, 2, 2] and (s["labels"][3:-3] == 1).all()
    for d in (s, p, i):
        assert d["vertices"].dtype == np.float64 and d["triangles"].dtype == np.int32


def test_a_dropped_carry_moves_every_kept_item_past_the_line():
    """The chunk loop of the integer block-sum scan restated in numpy on the keeps the device tests use: the honest loop
    gives the exclusive sums, and a carry lost at the second chunk moves every position past 2^20 — which the device tests
    compare for equality.  An array of no more than 1,024 tile sums does not know about the carry at all."""
    s, p = L.big("SHEET"), L.big("PREFIX")
    keep = L.random_keep(len(s["triangles"]))
    used = np.zeros(len(p["vertices"]), dtype=bool)
    used[p["triangles"].reshape(-1)] = True
    tail = np.zeros(len(s["triangles"]), dtype=bool)
    tail[0] = True
    tail[L.LINE - 3:] = True
    for tag, flags in (("SHEET random keep", keep), ("SHEET tail only", tail), ("PREFIX referenced vertices", used)):
        sums = L.tile_sums(flags)
        assert len(sums) == 1027 and int(sums.sum()) == int(flags.sum())
        want = np.cumsum(flags) - flags                       # the position of every item
        honest, total = L.block_sums_scan(sums)
        assert total == int(flags.sum()) and np.array_equal(honest.astype(np.int64), want[::L.TILE]), tag
        broken, broken_total = L.block_sums_scan(sums, carry_from_chunk=1)
        assert np.array_equal(broken[:L.CHUNK], honest[:L.CHUNK]) and (broken[L.CHUNK:] != honest[L.CHUNK:]).all(), tag
        assert broken_total == int(flags[L.LINE:].sum()) < total, tag
    short = L.tile_sums(np.ones(len(s["vertices"]), dtype=bool))
    assert len(short) == 515 and np.array_equal(L.block_sums_scan(short)[0], L.block_sums_scan(short, carry_from_chunk=1)[0])
    # four chunks: the carry is handed on three times, and losing it at any of them shows
    roots = (np.arange(len(L.big("ISOLATED")["vertices"])) % 3 == 0)
    sums = L.tile_sums(roots)
    honest, total = L.block_sums_scan(sums)
    assert len(sums) == 3085 and total == 1052677 and np.array_equal(honest.astype(np.int64), (np.cumsum(roots) - roots)[::L.TILE])
    for j in (1, 2, 3):
        broken = L.block_sums_scan(sums, carry_from_chunk=j)[0]
        assert np.array_equal(broken[:j * L.CHUNK], honest[:j * L.CHUNK]) and (broken[j * L.CHUNK:] != honest[j * L.CHUNK:]).all()


def test_the_vote_kernels_workgroup_loop_covers_every_pair_once():
    """the decomposition b -> (camera, point block) of the two vote cases: every pair once, the second trip holding the
    cameras the device tests look at; a loop that stops after one trip leaves exactly those out"""
    for n_points, n_cameras, first_second_trip_camera, n_second in ((5, 2 ** 20 + 261, 2 ** 20, 261), (257, 2 ** 19 + 3, 2 ** 19, 6)):
        nbp = (n_points + L.CV_THREADS - 1) // L.CV_THREADS
        c, p0 = L.vote_workgroups(n_points, n_cameras)
        assert len(c) == nbp * n_cameras == L.CV_MAX_BLOCKS + n_second
        pairs = c * nbp + p0 // L.CV_THREADS
        assert np.array_equal(pairs, np.arange(nbp * n_cameras)), "every (camera, point block) once"
        assert c[L.CV_MAX_BLOCKS:].min() == first_second_trip_camera and c[L.CV_MAX_BLOCKS:].max() == n_cameras - 1
        assert set(p0[L.CV_MAX_BLOCKS:].tolist()) == set(range(0, n_points, L.CV_THREADS)), "both point halves on the second trip"
        c1, _ = L.vote_workgroups(n_points, n_cameras, trips=1)
        assert len(c1) == L.CV_MAX_BLOCKS and c1.max() == first_second_trip_camera - 1
    c, p0 = L.vote_workgroups(816, 6)
    assert len(c) == 4 * 6 and c.tolist() == np.repeat(np.arange(6), 4).tolist(), "below the cap: one trip"


def test_the_area_bound_passes_the_device_order_and_fails_a_dropped_carry():
    """(T + 8) 2^-52 A separates the two by many orders of magnitude: the bound is no accident of the fixture"""
    areas = L.big("ISOLATED")["areas"]
    T = len(areas)
    ref = np.cumsum(areas)
    bound = L.area_scan_bound(areas)
    assert bound == (T + 8) * 2.0 ** -52 * float(areas.sum())
    honest = L.device_order_cumsum(areas)
    assert honest.shape == (T,) and (np.diff(honest) >= 0.0).all()
    worst = float(np.abs(honest - ref).max())
    # small: the device order on 2,500 items against a plain Python chain of the same association
    small = areas[:2500]
    got = L.device_order_cumsum(small)
    tile_off, k = 0.0, 0
    for b in range(L.tiles(len(small))):
        thread_off = 0.0
        for j in range(L.TILE_THREADS):
            run = 0.0
            for _ in range(L.TILE_ITEMS):
                if k < len(small):
                    run = run + float(small[k])
                    assert got[k] == tile_off + (thread_off + run), k
                    k += 1
            thread_off = thread_off + run
        tile_off = tile_off + thread_off
    assert k == len(small)
    broken = L.device_order_cumsum(areas, carry_from_chunk=1)
    assert np.array_equal(broken[:L.LINE], honest[:L.LINE]), "the first chunk does not know about the carry"
    worst_broken = float(np.abs(broken - ref).max())
    print(f"area scan, T = {T}: honest |device order - cumsum| = {worst / bound:.2e} of the bound, carry dropped at chunk 2: "
          f"{worst_broken / bound:.2e} of it")
    assert worst <= bound, "the honest order misses the bound"
    assert worst_broken > 1e6 * bound, "the bound cannot see a dropped carry"
    assert (np.abs(broken - ref)[L.LINE:] > bound).all(), "every item past 2^20 shows the dropped carry"
