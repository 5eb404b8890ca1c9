"""Mesh simplification on the device: vertex clustering on a uniform grid (csrc/mesh_simplify.hip through
`rnb_mesh_simplify_*`, include/rnbneus.h has the definition).  What every user of a 512^3 extraction does next — make the
mesh small enough to view, ship or bake — on the arrays marching cubes left on the GPU; there is no CPU path.

The vertices of one grid cell that valid triangles name become one vertex, which is one of them (the member nearest the
cell's mean): every output vertex is an input vertex, so attributes carry over by a gather and the vertices stay on the
iso-surface.  Triangles that collapse are dropped, and of the triangles that land on the same three cells only the first
survives.  Device and numpy (tests/mesh_simplify_ref.py) agree bit for bit."""
from __future__ import annotations

import ctypes as C
import math
import numbers

import torch

from . import native
from .mesh_args import check_attributes, check_mesh, finite_box

MAX_RESOLUTION = 2 ** 20 - 1     # cell indices are 21-bit
FLAG_BAD_INDEX, FLAG_BAD_VERTEX, FLAG_TABLE_FULL = 1, 2, 4
# what the renderer's `simplify=` may hold: the keywords of `simplify_mesh` that `check_arguments` checks
SIMPLIFY_KEYWORDS = ("cell_size", "target_triangles", "origin")


class _Pass:
    """One mesh, one workspace: count at a grid, then emit at the grid counted last."""

    def __init__(self, who, vts, tri):
        self.who, self.vts, self.tri = who, vts, tri
        self.V, self.T = vts.shape[0], tri.shape[0]
        self.dev = vts.device
        self.lib = native.load()
        self.ws = native.workspace("mesh_simplify", self.dev, self.V, self.T)
        self.counts = torch.empty(6, dtype=torch.int64, device=self.dev)
        self.grid = None

    def launch_count(self, origin, h):
        """the count stage, enqueued: no host read.  origin: three floats, or None = the device's default"""
        org = (C.c_double * 3)(*origin) if origin is not None else None
        self.grid = (org, float(h))
        with native.on_device(self.dev) as stream:
            native.check(self.lib.rnb_mesh_simplify_count(native.ptr(self.vts), self.V, native.ptr(self.tri), self.T, org,
                                                          float(h), native.ptr(self.ws), self.ws.numel(),
                                                          native.ptr(self.counts), stream))

    def count(self, origin, h):
        """counts [6] on the host (one synchronisation)"""
        self.launch_count(origin, h)
        c = [int(x) for x in self.counts.cpu()]
        if c[4] & FLAG_BAD_INDEX:
            raise ValueError(f"{self.who}: a triangle holds a vertex index outside [0, {self.V})")
        if c[4] & FLAG_TABLE_FULL:
            raise native.NativeError(f"{self.who}: a hash table filled up (its sizing excludes this)")
        return c

    def emit(self, nv, nt):
        org, h = self.grid
        v_out = torch.empty(nv, 3, dtype=torch.float64, device=self.dev)
        t_out = torch.empty(nt, 3, dtype=torch.int32, device=self.dev)
        v_index = torch.empty(nv, dtype=torch.int64, device=self.dev)
        v_cluster = torch.empty(self.V, dtype=torch.int32, device=self.dev)
        t_index = torch.empty(nt, dtype=torch.int64, device=self.dev)
        with native.on_device(self.dev) as stream:
            native.check(self.lib.rnb_mesh_simplify_emit(native.ptr(self.vts), self.V, native.ptr(self.tri), self.T, org, h,
                                                         native.ptr(self.ws), self.ws.numel(), nv, nt, native.ptr(v_out),
                                                         native.ptr(t_out), native.ptr(v_index), native.ptr(v_cluster),
                                                         native.ptr(t_index), stream))
        return v_out, t_out, v_index, v_cluster, t_index


def _result(v_out, t_out, v_index, v_cluster, t_index, attributes, info):
    return {"vertices": v_out, "triangles": t_out,
            "attributes": {k: a.index_select(0, v_index) for k, a in attributes.items()},
            "vertex_index": v_index, "vertex_cluster": v_cluster, "triangle_index": t_index, "info": info}


def _info(h, origin, V, T, c, tried):
    return {"cell_size": h, "origin": origin, "n_vertices": (V, c[0]), "n_triangles": (T, c[1]), "n_clusters": c[5],
            "n_degenerate": c[2], "n_duplicate": c[3],
            "skipped": {"bad_index": bool(c[4] & FLAG_BAD_INDEX), "bad_vertex": bool(c[4] & FLAG_BAD_VERTEX)}, "tried": tried}


def check_arguments(who, cell_size=None, target_triangles=None, origin=None):
    """ValueError for keywords that contradict themselves (`simplify_mesh`, the renderer's `simplify=`); the origin as
    three floats, or None"""
    if (cell_size is None) == (target_triangles is None):
        raise ValueError(f"{who}: give exactly one of cell_size and target_triangles")
    if cell_size is not None and not (isinstance(cell_size, numbers.Real) and not isinstance(cell_size, bool) and 0.0 < float(cell_size) < math.inf):
        raise ValueError(f"{who}: cell_size must be a positive finite number, not {cell_size!r}")
    if target_triangles is not None and (isinstance(target_triangles, bool) or int(target_triangles) != target_triangles
                                         or int(target_triangles) < 1):
        raise ValueError(f"{who}: target_triangles must be an integer >= 1, not {target_triangles!r}")
    if origin is None:
        return None
    o = [float(x) for x in (origin.tolist() if hasattr(origin, "tolist") else origin)]
    if len(o) != 3 or not all(math.isfinite(x) for x in o):
        raise ValueError(f"{who}: origin must be three finite numbers, not {origin!r}")
    return o


@torch.no_grad()
def simplify_mesh(vertices, triangles, *, cell_size=None, target_triangles=None, origin=None, attributes=None):
    """Simplifies a mesh by vertex clustering on a uniform grid, on the device.
    vertices [V,3] float64, triangles [T,3] int32 — the tensors `marching_cubes` / `clean_mesh` return.  Exactly one of
      `cell_size=h`: the cubic cells of the grid have side h (in the vertices' units; grid-index units = voxels for a
      marching-cubes mesh), or
      `target_triangles=n`: h = L / r with L the longest side of the box of the finite vertices and the integer resolution
      r bisected over [1, 2^20 - 1] with the count stage alone (at most 21 passes, each one host read, after one read of
      the box); returned is the emit for the largest r tried with 0 < T' <= n.  T'(r) is not strictly monotone: the
      promise is T' <= n and the list `info["tried"]` of (r, T'), not optimality.  A mesh with T <= n already comes back
      unchanged (apart from unreferenced vertices) with `tried == []`; ValueError when no r tried gives 0 < T' <= n.
    `origin`: three numbers, the corner of cell (0, 0, 0); default: per axis the minimum over the vertices with all-finite
    coordinates, computed on the device with no host read.
    `attributes`: dict of per-vertex device tensors [V, ...], gathered with `vertex_index`.
    Returns a dict: `vertices` [V',3] (input vertices, bit for bit), `triangles` [T',3] int32, `attributes`, `vertex_index`
    [V'] int64 (input index of every output vertex), `vertex_cluster` [V] int32 (output index of every input vertex's
    cluster, -1 when it has none), `triangle_index` [T'] int64 (input index of every surviving triangle) and `info`:
    `cell_size`, `origin` (device [3] float64), `n_vertices` / `n_triangles` as (before, after), `n_clusters`,
    `n_degenerate`, `n_duplicate`, `skipped` (`bad_index`, `bad_vertex`: a triangle was skipped for a non-finite vertex or
    one more than 2^20 cells from the origin — reported, not raised) and `tried`.
    ValueError for wrong shapes / dtypes and for a triangle index outside [0, V); RuntimeError for CPU tensors.  With
    `cell_size` one host synchronisation (the counts).  Never collective under `set_data_parallel`."""
    who = "simplify_mesh"
    org = check_arguments(who, cell_size, target_triangles, origin)
    if vertices is None:
        raise ValueError(f"{who}: vertices is None")
    V = check_mesh(who, triangles, None, vertices)
    attributes = check_attributes(who, attributes, V)
    dev = native.gpu_device(triangles, vertices, *attributes.values())
    tri, vts = triangles.detach().contiguous(), vertices.detach().contiguous()
    T = tri.shape[0]
    if target_triangles is None:
        run = _Pass(who, vts, tri)
        h = float(cell_size)
        c = run.count(org, h)
        origin_t = torch.tensor(org, dtype=torch.float64, device=dev) if org is not None else finite_box(vts)[0]
        return _result(*run.emit(c[0], c[1]), attributes, _info(h, origin_t, V, T, c, []))
    n = int(target_triangles)
    if T <= n:      # small enough already: only unreferenced vertices go
        from .mesh_clean import clean_mesh
        out = clean_mesh(vts, tri)
        index = out["vertex_index"]
        cluster = torch.full((V,), -1, dtype=torch.int32, device=dev)
        cluster[index] = torch.arange(index.shape[0], dtype=torch.int32, device=dev)
        nv = index.shape[0]
        info = _info(None, finite_box(vts)[0] if org is None else torch.tensor(org, dtype=torch.float64, device=dev), V, T,
                     [nv, T, 0, 0, 0, nv], [])
        return _result(out["vertices"], out["triangles"], index, cluster, torch.arange(T, dtype=torch.int64, device=dev),
                       attributes, info)
    lo_t, hi_t = finite_box(vts)
    box = torch.stack([lo_t, hi_t]).cpu()
    L = float((box[1] - box[0]).max())
    if not (0.0 < L < math.inf):
        raise ValueError(f"{who}: the finite vertices span a box of longest side {L}: no grid to bisect")
    if org is None:
        org = [float(x) for x in box[0]]
    run = _Pass(who, vts, tri)
    tried, seen = [], {}

    def count(r):
        c = run.count(org, L / r)
        tried.append((r, c[1]))
        seen[r] = c
        return c[1]

    lo, hi = 1, MAX_RESOLUTION
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if count(mid) <= n:
            lo = mid
        else:
            hi = mid - 1
    if lo not in seen:
        count(lo)
    good = [r for r, nt in tried if 0 < nt <= n]
    if not good:
        raise ValueError(f"{who}: no resolution tried gives between 1 and {n} triangles (tried (r, T'): {tried})")
    r = max(good)
    if tried[-1][0] != r:       # the workspace holds the grid counted last
        run.count(org, L / r)
    c = seen[r]
    info = _info(L / r, torch.tensor(org, dtype=torch.float64, device=dev), V, T, c, tried)
    info["resolution"] = r
    return _result(*run.emit(c[0], c[1]), attributes, info)
