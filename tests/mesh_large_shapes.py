"""Meshes and camera sets past 2^20 items, with analytic answers: what tests/test_gpu_mesh_second_trips.py runs on the
device and tests/test_mesh_large_shapes_host.py checks small on the host.  A helper, not a test module.

The integer scans of csrc/scan.hip.h work on tiles of TILE = 1,024 items, and the one workgroup that scans the tile sums
goes through them in chunks of CHUNK = 1,024 tiles: a scan takes the chunk loop's second trip only past 2^20 items.  The
area scan of csrc/mesh_eval.hip has the same geometry, and the vote kernel of csrc/mesh_cull.hip strides over its
workgroups past CV_MAX_BLOCKS = 2^20 of them.  Every builder takes its sizes as parameters, so the host test runs it
small; the three big instances are built once (`big`) and shared: callers must not modify them."""
import numpy as np

from tests import mesh_components_ref as MC
from tests import mesh_cull_ref as CU

TILE = 1024                    # kScanTile: items per tile (256 threads x 4)
TILE_THREADS, TILE_ITEMS = 256, 4
CHUNK = 1024                   # tile sums per trip of the block-sum kernels
LINE = TILE * CHUNK            # 2^20: the first item of the second chunk
CV_THREADS, CV_MAX_BLOCKS = 256, 1 << 20


def tiles(n):
    return (int(n) + TILE - 1) // TILE


def chunks(n):
    """trips of the chunk loop of a block-sum kernel over the tile sums of n items"""
    return (tiles(n) + CHUNK - 1) // CHUNK


# ---- the meshes -----------------------------------------------------------------------------------------------------
def sheet(m, k):
    """A height field of m x k quads: (m + 1)(k + 1) vertices row-major (vertex r (k + 1) + c), float64, with a gentle
    non-planar z; 2 m k triangles int32, quad by quad in row-major order, two per quad.  One component."""
    r, c = np.meshgrid(np.arange(m + 1), np.arange(k + 1), indexing="ij")
    x, y = 0.013 * c, 0.011 * r
    z = 0.02 * np.sin(0.05 * c) * np.cos(0.07 * r)
    v = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float64)
    qr, qc = np.meshgrid(np.arange(m), np.arange(k), indexing="ij")
    v00 = (qr * (k + 1) + qc).reshape(-1)
    v01, v10, v11 = v00 + 1, v00 + (k + 1), v00 + (k + 2)
    t = np.stack([np.stack([v00, v01, v11], axis=1), np.stack([v00, v11, v10], axis=1)], axis=1).reshape(-1, 3)
    assert v.shape == ((m + 1) * (k + 1), 3) and t.shape == (2 * m * k, 3), "the fixture moved"
    return np.ascontiguousarray(v), np.ascontiguousarray(t.astype(np.int32))


FLOATER = np.array([[0.0, 0.0, 0.0], [0.31, 0.0, 0.07], [0.0, 0.23, -0.05]])


def sheet_with_floaters(m, k):
    """`sheet(m, k)` between two isolated triangles: one in front (vertices 0..2, triangle 0) and one behind (the last
    three vertices, the last triangle).  Returns (vertices, triangles, labels): components are numbered by their smallest
    vertex index, so the labels are 0 (floater), 1 (sheet), 2 (floater)."""
    sv, st = sheet(m, k)
    V = len(sv) + 6
    v = np.concatenate([FLOATER + np.array([-1.0, -1.0, 0.7]), sv, FLOATER + np.array([11.0, 9.5, -0.6])])
    t = np.concatenate([[[0, 1, 2]], st + 3, [[V - 3, V - 2, V - 1]]]).astype(np.int32)
    labels = np.ones(V, dtype=np.int32)
    labels[:3], labels[-3:] = 0, 2
    return np.ascontiguousarray(v), np.ascontiguousarray(t), labels


def prefix(n_loose, m, k, seed=7):
    """n_loose vertices no triangle names (finite coordinates) followed by `sheet(m, k)`: (vertices, triangles)"""
    sv, st = sheet(m, k)
    loose = np.random.default_rng(seed).uniform(-3.0, 3.0, (n_loose, 3))
    return np.ascontiguousarray(np.concatenate([loose, sv])), np.ascontiguousarray((st + n_loose).astype(np.int32))


def isolated_labels(n_triangles):
    """labels of `mesh_components_ref.isolated(n)`: triangle j is component j"""
    return (np.arange(3 * n_triangles) // 3).astype(np.int32)


def random_keep(n_triangles, share=0.7, seed=5):
    """the per-triangle keep of the compaction tests: a random `share` of the triangles"""
    return np.random.default_rng(seed).uniform(size=n_triangles) < share


_BIG = {}


def big(name):
    """The three instances past 2^20, built once, as dicts:
    SHEET     sheet(725, 725) with floaters: V = 527,082 (515 tiles, one chunk), T = 1,051,252 (1,027 tiles, two chunks),
              2,676 triangles at indices >= 2^20; three components, `labels` analytic
    PREFIX    800,000 unreferenced vertices, then sheet(500, 500): V = 1,051,001 (1,027 tiles, two chunks), T = 500,000
              (489 tiles); 2,425 referenced vertices at indices >= 2^20; `n_loose`
    ISOLATED  mesh_components_ref.isolated(2^20 + 4096 + 5): T = 1,052,677 (1,029 tiles, 5 items in the last), V =
              3,158,031 (3,085 tiles, four chunks); C = T, `labels` = v // 3, `areas` (they span more than 10^6)"""
    if name in _BIG:
        return _BIG[name]
    if name == "SHEET":
        v, t, labels = sheet_with_floaters(725, 725)
        d = {"vertices": v, "triangles": t, "labels": labels}
        assert (len(v), len(t)) == (527082, 1051252) and (tiles(len(v)), tiles(len(t))) == (515, 1027), "the fixture moved"
        assert (chunks(len(v)), chunks(len(t))) == (1, 2) and len(t) - LINE == 2676, "the fixture moved"
    elif name == "PREFIX":
        v, t = prefix(800000, 500, 500)
        d = {"vertices": v, "triangles": t, "n_loose": 800000}
        assert (len(v), len(t)) == (1051001, 500000) and (tiles(len(v)), tiles(len(t))) == (1027, 489), "the fixture moved"
        assert (chunks(len(v)), chunks(len(t))) == (2, 1) and len(v) - LINE == 2425 and int(t.min()) == 800000, "the fixture moved"
    elif name == "ISOLATED":
        n = 2 ** 20 + 4096 + 5
        v, t = MC.isolated(n)
        v, t = np.ascontiguousarray(v), np.ascontiguousarray(t)
        areas, labels = MC.triangle_areas(v, t), isolated_labels(n)
        d = {"vertices": v, "triangles": t, "labels": labels, "areas": areas}
        assert (len(v), len(t)) == (3158031, 1052677) and (tiles(len(v)), tiles(len(t))) == (3085, 1029), "the fixture moved"
        assert (chunks(len(v)), chunks(len(t))) == (4, 2) and len(t) - (tiles(len(t)) - 1) * TILE == 5, "the fixture moved"
        share = float(areas[LINE:].sum() / areas.sum())
        assert len(t) - LINE == 4101 and areas.min() > 0.0 and areas.max() / areas.min() > 1e6, "the fixture moved"
        assert 0.0035 < share < 0.0045, f"the fixture moved: {share:.4%} of the area lies past triangle 2^20"
    else:
        raise KeyError(name)
    _BIG[name] = d
    return d


# ---- the integer block-sum scan and the vote kernel's workgroup loop, restated --------------------------------------------
def block_sums_scan(tile_sums, carry_from_chunk=None):
    """(exclusive offsets, total) of the tile sums as scan_block_sums_kernel (csrc/scan.hip.h) forms them: chunk by chunk
    of CHUNK sums, an exclusive scan inside the chunk plus the carry of the chunks before it.
    `carry_from_chunk=j`: the BROKEN scan that starts every chunk >= j from 0."""
    s = np.asarray(tile_sums, dtype=np.uint64)
    out = np.empty_like(s)
    carry = np.uint64(0)
    for base in range(0, len(s), CHUNK):
        if carry_from_chunk is not None and base // CHUNK >= carry_from_chunk:
            carry = np.uint64(0)
        part = s[base:base + CHUNK]
        inc = np.cumsum(part, dtype=np.uint64)
        out[base:base + CHUNK] = carry + inc - part
        carry = carry + (inc[-1] if len(inc) else np.uint64(0))
    return out, int(carry)


def tile_sums(flags):
    """per tile of TILE items the number of set flags"""
    f = np.asarray(flags).astype(np.uint64).reshape(-1)
    pad = np.zeros(tiles(len(f)) * TILE, dtype=np.uint64)
    pad[:len(f)] = f
    return pad.reshape(-1, TILE).sum(axis=1)


def vote_workgroups(n_points, n_cameras, trips=None):
    """The (camera, first point) of every virtual workgroup cv_kernel (csrc/mesh_cull.hip) visits, in the order of b:
    a grid of min(total, CV_MAX_BLOCKS) workgroups, each going over b = blockIdx, blockIdx + grid, ...  `trips=1`: the
    BROKEN loop that stops after its first trip."""
    nbp = (n_points + CV_THREADS - 1) // CV_THREADS
    total = nbp * n_cameras
    grid = min(total, CV_MAX_BLOCKS)
    n_trips = (total + grid - 1) // grid if trips is None else trips
    b = np.concatenate([np.arange(k * grid, min((k + 1) * grid, total), dtype=np.int64) for k in range(n_trips)])
    c = b // nbp
    return c, (b - c * nbp) * CV_THREADS


# ---- the area scan in the device's association ------------------------------------------------------------------------
def device_order_cumsum(areas, carry_from_chunk=None):
    """The inclusive area sums as csrc/mesh_eval.hip associates them: inside a thread its TILE_ITEMS items in sequence
    from 0, across the TILE_THREADS threads of a tile in sequence, across the tile sums in sequence (the chain goes on
    across chunks of CHUNK tiles through `carry`); C_t = tile offset + (thread offset + the thread's running sum).
    `carry_from_chunk=j`: the BROKEN scan whose carry is lost (reset to 0) at the start of every chunk >= j."""
    a = np.asarray(areas, dtype=np.float64).reshape(-1)
    T = len(a)
    nt = tiles(T)
    x = np.zeros(nt * TILE)
    x[:T] = a
    x = x.reshape(nt, TILE_THREADS, TILE_ITEMS)
    run = np.empty_like(x)
    acc = np.zeros((nt, TILE_THREADS))
    for k in range(TILE_ITEMS):
        acc = acc + x[:, :, k]
        run[:, :, k] = acc
    t_off = np.empty((nt, TILE_THREADS))
    off = np.zeros(nt)
    for j in range(TILE_THREADS):
        t_off[:, j] = off
        off = off + acc[:, j]
    tile_total = off
    b_off = np.empty(nt)
    carry = 0.0
    for b in range(nt):
        if carry_from_chunk is not None and b % CHUNK == 0 and b // CHUNK >= carry_from_chunk:
            carry = 0.0
        b_off[b] = carry
        carry = carry + float(tile_total[b])
    cum = b_off[:, None, None] + (t_off[:, :, None] + run)
    return cum.reshape(-1)[:T]


def area_scan_bound(areas):
    """(T + 8) 2^-52 A: two summation orders of T non-negative terms each lie within (T - 1) 2^-53 A of the exact sum,
    and 8 x 2^-52 A covers a few ulps of area evaluation per triangle"""
    a = np.asarray(areas, dtype=np.float64)
    return (len(a) + 8) * 2.0 ** -52 * float(a.sum())


# ---- the votes of one point under many cameras ------------------------------------------------------------------------
def votes_one_point(point, projections, masks, size):
    """`mesh_cull_ref.frame_status` vectorised over the cameras for ONE point: (reaches [C] bool, status [C] uint8 for the
    others, px, py).  The same comparisons in the same order, and numpy does each operation once per element, so the result
    is bit-identical to the per-camera loop.  projections [C,3,4], masks [C,H,W] or None, size = (H, W)."""
    H, W = size
    pt = np.asarray(point, dtype=np.float64).reshape(1, 3)
    P = np.asarray(projections, dtype=np.float64).reshape(-1, 3, 4)
    C = len(P)
    x, y, w = CU.project(pt, P.transpose(1, 2, 0))                      # P[r, k] is [C], X is [1]: each result is [C]
    ok = np.isfinite(pt).all() & np.isfinite(w) & (w > 0.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        a, b = x / w + 0.5, y / w + 0.5
        inside = ok & (a >= 0.0) & (a < float(W)) & (b >= 0.0) & (b < float(H))
    px = np.where(inside, np.floor(np.where(inside, a, 0.0)), 0).astype(np.int64)
    py = np.where(inside, np.floor(np.where(inside, b, 0.0)), 0).astype(np.int64)
    status = np.full(C, CU.OUT_OF_FRAME, dtype=np.uint8)
    reaches = inside.copy()
    if masks is not None:
        off = inside & (np.asarray(masks)[np.arange(C), py, px] == 0)
        status[off] = CU.OUTSIDE_MASK
        reaches &= ~off
    return reaches, status, px, py


def shifted_cameras(n_cameras, seed, size=(16, 16), p_mask=0.6):
    """(projections [C,3,4], masks [C,H,W] uint8) of the vote tests: P_c = [[1,0,8+dx,0],[0,1,8+dy,0],[0,0,1,0]] with dx,
    dy uniform in [-12, 12], every eye at the origin; random mask bits with P(1) = p_mask (drawn 65,536 cameras at a
    time: the masks themselves are the largest array)"""
    rng = np.random.default_rng(seed)
    H, W = size
    P = np.zeros((n_cameras, 3, 4))
    P[:, 0, 0] = P[:, 1, 1] = P[:, 2, 2] = 1.0
    P[:, 0, 2] = 8.0 + rng.uniform(-12.0, 12.0, n_cameras)
    P[:, 1, 2] = 8.0 + rng.uniform(-12.0, 12.0, n_cameras)
    masks = np.empty((n_cameras, H, W), dtype=np.uint8)
    for c0 in range(0, n_cameras, 65536):
        part = masks[c0:c0 + 65536]
        part[...] = rng.random(part.shape, dtype=np.float32) < p_mask
    return P, masks


# the two parallel triangles of tests/test_gpu_mesh_cull.py test_occlusion_on_two_parallel_triangles and three of its points
# (hidden by the small triangle, past its edge, in front of both), then a point with a NaN coordinate and one behind
# every camera (Z < 0, so w < 0)
TWO_TRIANGLES_V = np.array([[-4.0, -4.0, 2.0], [8.0, -4.0, 2.0], [-4.0, 8.0, 2.0], [-0.25, -0.25, 1.0], [0.5, -0.25, 1.0],
                            [-0.25, 0.5, 1.0]])
TWO_TRIANGLES_T = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)
VOTE_POINTS = np.array([[0.0, 0.0, 2.0], [1.0, 1.0, 2.0], [0.1, 0.1, 0.5], [0.3, np.nan, 1.0], [0.2, 0.1, -1.5]])


def vote_points(n, seed=0):
    """VOTE_POINTS, then n - 5 random points on either side of the two triangles (every 16th behind the cameras)"""
    rng = np.random.default_rng(seed)
    more = np.stack([rng.uniform(-1.5, 1.5, n - 5), rng.uniform(-1.5, 1.5, n - 5), rng.uniform(0.25, 3.0, n - 5)], axis=1)
    more[::16, 2] *= -1.0
    return np.ascontiguousarray(np.concatenate([VOTE_POINTS, more]))


def seen_from_the_origin(points):
    """What the segment origin -> point meets, per point [N] uint8: SEEN / OCCLUDED past the two triangles, OUT_OF_FRAME for
    a point no camera casts (a non-finite coordinate, Z <= 0).  With every eye at the origin the segment does not depend on
    the camera, so ONE call of `mesh_cull_ref.view_votes` with one camera that has every other point in its frame answers
    for all of them."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    wide = np.array([[[1.0, 0.0, 32.0, 0.0], [0.0, 1.0, 32.0, 0.0], [0.0, 0.0, 1.0, 0.0]]])       # x / z + 32 in a 64 x 64 frame
    st = CU.view_votes(pts, wide, np.zeros((1, 3)), None, (64, 64), TWO_TRIANGLES_V, TWO_TRIANGLES_T, occlusion=True)[0][0]
    castable = np.isfinite(pts).all(axis=1) & (pts[:, 2] > 0.0)
    assert (st[castable] >= CU.OCCLUDED).all() and (st[~castable] == CU.OUT_OF_FRAME).all(), "the wide camera misses a point"
    return st
