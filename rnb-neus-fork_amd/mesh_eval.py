"""Mesh evaluation on the device: exact closest points on a triangle mesh, area-weighted surface samples, and the
mesh-to-mesh measures built from them — accuracy, completeness, Chamfer, sampled Hausdorff, precision / recall / F-score
(csrc/mesh_eval.hip through `rnb_mesh_bins_*`, `rnb_mesh_closest_points`, `rnb_mesh_sample_*`, include/rnbneus.h).  The
arrays stay where marching cubes and the cleanup left them; there is no CPU path.

Distances are point-to-TRIANGLE, not point-to-sample: `MeshIndex.closest` returns, for every query, the minimum over all
triangles of the mesh under the order (squared distance, triangle index), bit-equal from run to run and whatever the grid.
A triangle with a non-finite vertex is skipped (`MeshIndex.skipped`); an index outside [0, V) is a ValueError."""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import mesh_cull, mesh_raycast, native
from .mesh_args import check_mesh, check_points, finite_box

_MAX_CELLS = native.MESH_BINS_MAX_CELLS
_COARSEN_ROUNDS = 8


def _check_cells(who, cells):
    if cells is None:
        return None
    dims = tuple(cells) if isinstance(cells, (tuple, list)) else (cells,) * 3
    if len(dims) != 3 or any(not isinstance(d, int) or isinstance(d, bool) or d < 1 for d in dims):
        raise ValueError(f"{who}: cells must be a positive int or three of them, not {cells!r}")
    if dims[0] * dims[1] * dims[2] > _MAX_CELLS:
        raise ValueError(f"{who}: cells = {cells!r} is more than 2^24 cells")
    return dims


def default_grid(extent, n_triangles):
    """(dims, cell_size) of the default bins for a box of the given extent (three floats >= 0): cubic cells, about
    max(T, 1) / 2 of them (marching-cubes triangles are about a cell wide then, and a cell holds a handful), at most 2^24."""
    target = min(max(int(n_triangles), 1) // 2, _MAX_CELLS)
    ext = [float(e) for e in extent]
    pos = [e for e in ext if e > 0.0]
    if not pos:
        return (1, 1, 1), 1.0
    if target <= 1:
        return (1, 1, 1), max(pos) * (1.0 + 2.0 ** -40)
    cell = math.prod(pos) ** (1.0 / len(pos)) / target ** (1.0 / len(pos))
    while True:
        dims = tuple(int(e / cell) + 1 for e in ext)
        if dims[0] * dims[1] * dims[2] <= _MAX_CELLS:
            return dims, cell
        cell *= 1.25


def forced_grid(extent, dims):
    """cell_size of bins with the given dims over a box of the given extent: the smallest cubic cell that covers it"""
    cell = max(float(e) / d for e, d in zip(extent, dims)) * (1.0 + 2.0 ** -40)
    return cell if cell > 0.0 else 1.0


class MeshIndex:
    """Triangle bins of one mesh, built once, serving many closest-point queries.
    vertices [V,3] float64, triangles [T,3] int32 (device tensors, what `marching_cubes` / `clean_mesh` return).
    `cells`: None = cubic cells with n_cells ~ max(T, 1) / 2 (at most 2^24); if the mesh then needs more than
    16 T + n_cells entries (a few huge triangles over many cells) the dims are halved and the mesh is counted again, at
    most 8 times, after which ONE cell is used (E <= T: brute force).  An int or a 3-tuple forces the dims (no coarsening).
    Attributes: `dims`, `cell_size`, `origin` (floats), `n_cells`, `n_entries` (E), `rounds` (counting passes), `skipped`
    (True when a triangle with a non-finite vertex was left out), `covers` (the grid's box holds every binned triangle:
    always, for the grids built here; the query's bound uses it), `n_triangles`, `n_vertices`.
    `grid=(origin, cell_size, dims)` places the bins by hand (any box, covering the mesh or not: what lies outside goes
    to the boundary cells, and no result of `closest` changes), without coarsening.  `raycast`, `interpolate` and `visible`
    (mesh_raycast.py) and `view_votes` (mesh_cull.py) cast rays at the same bins; they need `covers`.
    ValueError for wrong shapes / dtypes and for a triangle index outside [0, V); RuntimeError for CPU tensors.
    Host synchronisations: one for the bounding box, one per counting pass."""

    def __init__(self, vertices, triangles, cells=None, grid=None):
        who = "MeshIndex"
        V = check_mesh(who, triangles, None, vertices)
        forced = _check_cells(who, cells)
        if grid is not None:
            if cells is not None:
                raise ValueError(f"{who}: give cells or grid, not both")
            g_origin, g_cell, g_dims = grid
            g_origin, g_cell, forced = [float(x) for x in g_origin], float(g_cell), _check_cells(who, tuple(g_dims))
            if len(g_origin) != 3 or not all(math.isfinite(x) for x in g_origin) or not (g_cell > 0.0 and math.isfinite(g_cell)):
                raise ValueError(f"{who}: grid = (origin, cell_size, dims) needs a finite origin and a positive cell size")
        dev = native.gpu_device(triangles, vertices)
        lib = native.load()
        self.vertices = vertices.detach().contiguous()
        self.triangles = triangles.detach().contiguous()
        self.n_vertices, self.n_triangles, self.device = V, self.triangles.shape[0], dev
        T = self.n_triangles
        bad = ((self.triangles < 0) | (self.triangles >= V)).any().to(torch.float64).reshape(1, 1).expand(1, 3)
        host = torch.cat([torch.stack(finite_box(self.vertices)), bad]).cpu()     # (the box and the flag in one read)
        if float(host[2, 0]) != 0.0:
            raise ValueError(f"{who}: a triangle holds a vertex index outside [0, {V})")
        lo, hi = host[0].tolist(), host[1].tolist()
        extent = [h - l for l, h in zip(lo, hi)]
        if not all(math.isfinite(e) for e in extent):
            raise ValueError(f"{who}: the mesh's bounding box overflows float64")
        if grid is not None:
            lo, dims, cell = g_origin, forced, g_cell
        elif forced is not None:
            dims, cell = forced, forced_grid(extent, forced)
        else:
            dims, cell = default_grid(extent, T)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        rounds = 0
        while True:
            rounds += 1
            n_cells = dims[0] * dims[1] * dims[2]
            bins = native.MeshBins((C.c_double * 3)(*lo), cell, (C.c_int32 * 3)(*dims), 0)
            ws = native.workspace("mesh_bins", dev, n_cells)
            cell_start = torch.empty(n_cells + 1, dtype=torch.int64, device=dev)
            with native.on_device(dev) as stream:
                native.check(lib.rnb_mesh_bins_count(native.ptr(self.vertices), V, native.ptr(self.triangles), T, C.byref(bins),
                                                     native.ptr(ws), ws.numel(), native.ptr(cell_start), native.ptr(counts),
                                                     stream))
            E, bits = (int(c) for c in counts.cpu())
            if forced is not None or n_cells == 1 or E <= 16 * T + n_cells:
                break
            if rounds > _COARSEN_ROUNDS:
                dims, cell = (1, 1, 1), forced_grid(extent, (1, 1, 1))
            else:
                dims, cell = tuple((d + 1) // 2 for d in dims), cell * 2.0
        if E > 2 ** 31 - 1:
            raise ValueError(f"{who}: {E} bin entries for cells = {dims}: use fewer cells")
        self.entries = torch.empty(E, dtype=torch.int32, device=dev)
        self.corners = torch.empty(T, 9, dtype=torch.float64, device=dev)
        with native.on_device(dev) as stream:
            native.check(lib.rnb_mesh_bins_emit(native.ptr(self.vertices), V, native.ptr(self.triangles), T, C.byref(bins),
                                                native.ptr(ws), ws.numel(), native.ptr(cell_start), E, native.ptr(self.entries),
                                                native.ptr(self.corners), stream))
        self.bins, self.cell_start = bins, cell_start
        self.dims, self.cell_size, self.origin, self.n_cells = tuple(dims), float(cell), tuple(lo), n_cells
        self.n_entries, self.rounds = E, rounds
        self.skipped, self.covers = bool(bits & native.MESH_BINS_SKIPPED), not bits & native.MESH_BINS_OUTSIDE
        self._origin_t = torch.tensor(lo, dtype=torch.float64, device=dev)
        self._dims_t = torch.tensor(dims, dtype=torch.float64, device=dev)

    def native_args(self):
        """the six arguments by which the native calls take these bins: the grid, the cells' first entries, the entries and
        their count, the triangles' corners and their count"""
        return (C.byref(self.bins), native.ptr(self.cell_start), native.ptr(self.entries), self.n_entries,
                native.ptr(self.corners), self.n_triangles)

    def _cell_order(self, q):
        """the permutation that sorts the queries by cell: neighbouring lanes of the query kernel then read the same entries
        (locality only: no result depends on it)"""
        big = torch.finfo(torch.float64).max
        c = torch.floor((torch.nan_to_num(q, nan=0.0, posinf=big, neginf=-big) - self._origin_t) / self.cell_size)
        c = torch.minimum(torch.clamp(c, min=0.0), self._dims_t - 1.0).to(torch.int64)
        return torch.argsort((c[:, 2] * self.dims[1] + c[:, 1]) * self.dims[0] + c[:, 0])

    @torch.no_grad()
    def closest(self, points):
        """The closest point of the mesh to every row of points [N,3] float64 (same device).  Returns a dict of device
        tensors: `dist2` [N] float64 (the squared distance as computed), `distance` = sqrt(dist2), `closest` [N,3] float64,
        `triangle` [N] int32 (ties to the smaller index).  A query with a non-finite coordinate: NaN, NaN, -1; a mesh without
        a usable triangle: +inf, NaN, -1.  No host synchronisation."""
        who = "MeshIndex.closest"
        check_points(who, "points", points, dtypes=(torch.float64,), noun="points")
        dev = native.gpu_device(points)
        if dev != self.device:
            raise RuntimeError(f"{who}: points live on {dev}, the mesh on {self.device}")
        q = points.detach().contiguous()
        N = q.shape[0]
        dist2 = torch.empty(N, dtype=torch.float64, device=dev)
        closest = torch.empty(N, 3, dtype=torch.float64, device=dev)
        triangle = torch.empty(N, dtype=torch.int32, device=dev)
        if N > 0:
            order = self._cell_order(q)
            qs = q.index_select(0, order)
            d2s, cls, trs = torch.empty_like(dist2), torch.empty_like(closest), torch.empty_like(triangle)
            with native.on_device(dev) as stream:
                native.check(native.load().rnb_mesh_closest_points(
                    native.ptr(qs), N, *self.native_args(), native.MESH_BINS_COVER if self.covers else 0,
                    native.ptr(d2s), native.ptr(cls), native.ptr(trs), stream))
            dist2[order], closest[order], triangle[order] = d2s, cls, trs
        return {"distance": torch.sqrt(dist2), "dist2": dist2, "closest": closest, "triangle": triangle}

    def raycast(self, origins, directions, t_min=None, t_max=None):
        """The first hit of every ray with the mesh: `mesh_raycast.raycast` has the contract."""
        return mesh_raycast.raycast(self, origins, directions, t_min, t_max)

    def interpolate(self, hits, vertex_values):
        """Per-vertex values at the hits of `raycast`, barycentrically: `mesh_raycast.interpolate`."""
        return mesh_raycast.interpolate(self, hits, vertex_values)

    def visible(self, points, eye, rel_tol=mesh_raycast.VISIBLE_REL_TOL):
        """Which points the eye sees past the mesh: `mesh_raycast.visible`."""
        return mesh_raycast.visible(self, points, eye, rel_tol)

    def view_votes(self, points, projections, eyes, masks=None, *, image_size=None, occlusion=True,
                   rel_tol=mesh_raycast.VISIBLE_REL_TOL, return_status=False):
        """Per point how many cameras have it out of frame, outside the mask, occluded, seen: `mesh_cull.view_votes`."""
        return mesh_cull.view_votes(self, points, projections, eyes, masks, image_size=image_size, occlusion=occlusion,
                                    rel_tol=rel_tol, return_status=return_status)


@torch.no_grad()
def sample_surface(vertices, triangles, n, seed=0):
    """n points on the surface of a mesh, area-weighted and deterministic (systematic sampling: triangle t receives
    n A_t / A samples up to rounding; the same seed gives the same bits; include/rnbneus.h has the integer mixer).
    vertices [V,3] float64, triangles [T,3] int32 on the device.  Returns a dict of device tensors: `points` [n,3] float64,
    `triangle` [n] int32, `bary` [n,3] float64 (>= 0, sum 1; points = sum of bary x corner) and `normal` [n,3] float64 (the
    unit face normal; zero when undefined), and `area` (float: the total area A).
    ValueError for wrong shapes / dtypes, a triangle index outside [0, V), n < 0, or a total area that is zero or not
    finite; RuntimeError for CPU tensors.  One host synchronisation (A with the bad-index flag)."""
    who = "sample_surface"
    V = check_mesh(who, triangles, None, vertices)
    if isinstance(n, bool) or int(n) != n or not 0 <= int(n) <= 2 ** 31 - 1:
        raise ValueError(f"{who}: n must be an integer in [0, 2^31 - 1], not {n!r}")
    if isinstance(seed, bool) or int(seed) != seed:
        raise ValueError(f"{who}: seed must be an integer, not {seed!r}")
    n = int(n)
    seed = int(seed) & (2 ** 64 - 1)
    seed = seed - 2 ** 64 if seed >= 2 ** 63 else seed
    dev = native.gpu_device(triangles, vertices)
    lib = native.load()
    vts, tri = vertices.detach().contiguous(), triangles.detach().contiguous()
    T = tri.shape[0]
    ws = native.workspace("mesh_sample", dev, T)
    cum = torch.empty(T, dtype=torch.float64, device=dev)
    head = torch.empty(2, dtype=torch.float64, device=dev)     # A, the bad-index flag
    with native.on_device(dev) as stream:
        native.check(lib.rnb_mesh_sample_areas(native.ptr(vts), V, native.ptr(tri), T, native.ptr(ws), ws.numel(),
                                               native.ptr(cum), native.ptr(head), stream))
    head[1] = ((tri < 0) | (tri >= V)).any()
    area, bad = head.cpu().tolist()
    if bad:
        raise ValueError(f"{who}: a triangle holds a vertex index outside [0, {V})")
    if not (area > 0.0 and math.isfinite(area)):
        raise ValueError(f"{who}: the total area of the mesh is {area}: nothing to sample")
    out = {"points": torch.empty(n, 3, dtype=torch.float64, device=dev),
           "triangle": torch.empty(n, dtype=torch.int32, device=dev),
           "bary": torch.empty(n, 3, dtype=torch.float64, device=dev),
           "normal": torch.empty(n, 3, dtype=torch.float64, device=dev)}
    with native.on_device(dev) as stream:
        native.check(lib.rnb_mesh_sample_surface(native.ptr(vts), V, native.ptr(tri), T, native.ptr(cum), native.ptr(head), n,
                                                 seed, native.ptr(out["points"]), native.ptr(out["triangle"]),
                                                 native.ptr(out["bary"]), native.ptr(out["normal"]), stream))
    out["area"] = area
    return out


def distance_statistics(dist_a, dist_b, thresholds=()):
    """The statistics of `mesh_distance` from the two distance arrays (a-samples to b, b-samples to a), as ONE device
    tensor [6 + 2 n_thresholds] float64: mean, rms, max of a; mean, rms, max of b; then per threshold the fraction of a
    and of b strictly below it.  Torch reductions only."""
    rows = []
    for d in (dist_a, dist_b):
        rows += [d.mean(), torch.sqrt((d * d).mean()), d.max()]
    for tau in thresholds:
        rows += [(dist_a < tau).to(torch.float64).mean(), (dist_b < tau).to(torch.float64).mean()]
    return torch.stack(rows)


@torch.no_grad()
def mesh_distance(va, ta, vb, tb, n_samples=1_000_000, thresholds=(), seed=0, return_samples=False):
    """Mesh a (vertices va, triangles ta) against the reference mesh b, both in the same coordinates, on the device.
    `n_samples` area-weighted points are drawn on each surface (`sample_surface`, seed for a and seed + 1 for b) and sent
    to the other mesh's `MeshIndex.closest`: point-to-triangle distances, exact for the samples drawn.  Returns floats:
      `accuracy`      mean distance of the a-samples to b         `rms_accuracy`, `max_accuracy`: their rms and maximum
      `completeness`  mean distance of the b-samples to a         `rms_completeness`, `max_completeness`
      `chamfer`       (accuracy + completeness) / 2               `hausdorff`: max(max_accuracy, max_completeness), sampled
      `thresholds` and, per threshold tau in that order, tuples `precision` (fraction of a-samples with distance < tau),
      `recall` (of b-samples) and `fscore` = 2 P R / (P + R), 0 when both are 0.
    All statistics are torch reductions gathered into one tensor and read with ONE host synchronisation (building the two
    indices and drawing the samples have their own: see `MeshIndex`, `sample_surface`).  `return_samples`: also
    `samples_a`, `samples_b` [n,3] and `distance_a`, `distance_b` [n] as device tensors."""
    who = "mesh_distance"
    if isinstance(n_samples, bool) or int(n_samples) != n_samples or int(n_samples) < 1:
        raise ValueError(f"{who}: n_samples must be an integer >= 1, not {n_samples!r}")
    thresholds = tuple(float(t) for t in thresholds)
    if any(not t >= 0.0 for t in thresholds):
        raise ValueError(f"{who}: thresholds must be >= 0, not {thresholds!r}")
    check_mesh(who, ta, None, va)
    check_mesh(who, tb, None, vb)
    index_a, index_b = MeshIndex(va, ta), MeshIndex(vb, tb)
    if index_a.device != index_b.device:
        raise RuntimeError(f"{who}: the meshes live on different devices ({index_a.device} and {index_b.device})")
    pa = sample_surface(va, ta, int(n_samples), seed)["points"]
    pb = sample_surface(vb, tb, int(n_samples), int(seed) + 1)["points"]
    da, db = index_b.closest(pa)["distance"], index_a.closest(pb)["distance"]
    s = distance_statistics(da, db, thresholds).cpu().tolist()
    out = {"accuracy": s[0], "rms_accuracy": s[1], "max_accuracy": s[2], "completeness": s[3], "rms_completeness": s[4],
           "max_completeness": s[5], "chamfer": 0.5 * (s[0] + s[3]), "hausdorff": max(s[2], s[5]), "n_samples": int(n_samples),
           "thresholds": thresholds, "precision": tuple(s[6::2]), "recall": tuple(s[7::2])}
    out["fscore"] = tuple(2.0 * p * r / (p + r) if p + r > 0.0 else 0.0 for p, r in zip(out["precision"], out["recall"]))
    if return_samples:
        out.update(samples_a=pa, samples_b=pb, distance_a=da, distance_b=db)
    return out
