"""Mesh cleanup on the device: connected components, floater removal, compaction (csrc/mesh_clean.hip through
`rnb_mesh_*`, include/rnbneus.h).  The first step after `validate_mesh` in every NeuS-family workflow — keep the largest
component, or drop the small ones — on the arrays marching cubes left on the GPU; there is no CPU path.

Connectivity: two vertices are connected when some triangle names both.  Components are numbered 0..C-1 in increasing
order of their smallest vertex index; a vertex no triangle names has label -1 and is always dropped by cleaning.
`compact_triangles` is the same compaction by a per-triangle keep (what `mesh_cull.cull_mesh` ends with)."""
from __future__ import annotations

import torch

from . import native
from .mesh_args import check_attributes, check_mesh

_BY = ("area", "triangles")
# what the renderer's `clean=` may hold: the selection keywords of `clean_mesh` (checked by `check_criteria`)
CLEAN_KEYWORDS = ("by", "keep_largest", "min_fraction", "min_triangles")


def _components(who, triangles, V, vertices):
    """labels, C, the statistics and the workspace.  One host synchronisation: C with the bad-index flag."""
    dev = native.gpu_device(triangles, vertices)
    lib = native.load()
    tri = triangles.detach().contiguous()
    vts = vertices.detach().contiguous() if vertices is not None else None
    T = tri.shape[0]
    ws = native.workspace("mesh_clean", dev, V, T)
    labels = torch.empty(V, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    with native.on_device(dev) as stream:
        native.check(lib.rnb_mesh_components(native.ptr(tri), T, V, native.ptr(ws), ws.numel(), native.ptr(labels),
                                             native.ptr(counts), stream))
    n_comp, bad = (int(c) for c in counts.cpu())
    if bad:
        raise ValueError(f"{who}: a triangle holds a vertex index outside [0, {V})")
    out = {"labels": labels, "n_components": n_comp,
           "triangles": torch.empty(n_comp, dtype=torch.int64, device=dev),
           "vertices": torch.empty(n_comp, dtype=torch.int64, device=dev)}
    if vts is not None:
        out["area"] = torch.empty(n_comp, dtype=torch.float64, device=dev)
        out["bbox_min"] = torch.empty(n_comp, 3, dtype=torch.float64, device=dev)
        out["bbox_max"] = torch.empty(n_comp, 3, dtype=torch.float64, device=dev)
    with native.on_device(dev) as stream:
        native.check(lib.rnb_mesh_component_stats(native.ptr(tri), T, native.ptr(vts), V, native.ptr(labels), n_comp,
                                                  native.ptr(ws), ws.numel(), native.ptr(out["triangles"]),
                                                  native.ptr(out["vertices"]), native.ptr(out.get("area")),
                                                  native.ptr(out.get("bbox_min")), native.ptr(out.get("bbox_max")), stream))
    return out, tri, vts, ws


@torch.no_grad()
def mesh_components(triangles, n_vertices=None, vertices=None):
    """Connected components of a triangle mesh on the device.
    triangles [T,3] int32; `n_vertices` = V, or `vertices` [V,3] float64 (then the geometric statistics come too).
    Returns a dict of device tensors: `labels` [V] int32 (component of every vertex, -1 = unreferenced), `n_components`
    (int C), `triangles` [C] and `vertices` [C] int64 (sizes of the components) and, with coordinates, `area` [C] float64
    (sum of triangle areas, bit-reproducible from run to run: integer accumulation, no floating-point atomics),
    `bbox_min`, `bbox_max` [C,3] float64.  A component with a NaN coordinate has a NaN area.
    ValueError for wrong shapes / dtypes and for a triangle index outside [0, V); RuntimeError for CPU tensors.  One host
    synchronisation.  Never collective under `set_data_parallel`."""
    V = check_mesh("mesh_components", triangles, n_vertices, vertices)
    return _components("mesh_components", triangles, V, vertices)[0]


def check_criteria(who, by="area", keep_largest=None, min_fraction=None, min_triangles=None, has_vertices=True):
    """ValueError for selection keywords that contradict themselves (`clean_mesh`, the renderer's `clean=`)"""
    if by not in _BY:
        raise ValueError(f"{who}: by must be one of {_BY}, not {by!r}")
    if by == "area" and not has_vertices:
        raise ValueError(f"{who}: by='area' needs the vertex coordinates")
    if keep_largest is not None and (int(keep_largest) != keep_largest or int(keep_largest) < 1):
        raise ValueError(f"{who}: keep_largest must be an integer >= 1, not {keep_largest!r}")
    if min_fraction is not None and not 0.0 <= float(min_fraction) <= 1.0:
        raise ValueError(f"{who}: min_fraction must lie in [0, 1], not {min_fraction!r}")
    if min_triangles is not None and (int(min_triangles) != min_triangles or int(min_triangles) < 0):
        raise ValueError(f"{who}: min_triangles must be an integer >= 0, not {min_triangles!r}")


def select_components(measure, n_triangles, keep_largest=None, min_fraction=None, min_triangles=None):
    """The keep mask [C] bool of `clean_mesh` from the components' measure (area or triangle count) and triangle counts:
    the criteria given are ANDed; `keep_largest=k` keeps the k largest measures, ties to the smaller id; `min_fraction=f`
    keeps measure >= f x the largest; a NaN measure ranks below every number and passes no `min_fraction`.  Device
    tensors in, device tensor out, no host synchronisation."""
    n = measure.shape[0]
    keep = torch.ones(n, dtype=torch.bool, device=measure.device)
    if n == 0:
        return keep
    m = measure.to(torch.float64)
    ranked = torch.where(torch.isnan(m), torch.full_like(m, float("-inf")), m)
    if keep_largest is not None:
        order = torch.sort(ranked, descending=True, stable=True).indices[:int(keep_largest)]
        top = torch.zeros_like(keep)
        top[order] = True
        keep &= top
    if min_fraction is not None:
        keep &= m >= float(min_fraction) * ranked.max()
    if min_triangles is not None:
        keep &= n_triangles >= int(min_triangles)
    return keep


@torch.no_grad()
def clean_mesh(vertices, triangles, *, by="area", keep_largest=None, min_fraction=None, min_triangles=None,
               attributes=None):
    """Keeps the selected connected components of a mesh and compacts it, on the device.
    vertices [V,3] float64, triangles [T,3] int32 — the tensors `marching_cubes` returns.
    Selection (criteria given are ANDed): `by` = "area" (default) or "triangles" is the measure; `keep_largest=k` keeps
    the k components with the largest measure (ties to the smaller id); `min_fraction=f` those with measure >= f x the
    largest; `min_triangles=n` those with at least n triangles.  With none given only unreferenced vertices go, so a
    marching-cubes mesh comes back unchanged bit for bit.
    `attributes`: dict of per-vertex device tensors [V, ...] (normals, colours, albedo, sdf), gathered with the same map.
    Compaction is stable: the result equals `vertices[keep]` and `newidx[triangles[keep_t]]`.
    Returns a dict: `vertices` [V',3], `triangles` [T',3], `attributes` (dict), `vertex_index` [V'] int64 (old index of
    every kept vertex) and `info`: `n_components`, `by`, `kept` (ids, device int64), `measure` [C] and `measure_kept`,
    `n_vertices` / `n_triangles` as (before, after).
    Two host synchronisations (C; then V' and T').  Never collective under `set_data_parallel`."""
    who = "clean_mesh"
    check_criteria(who, by, keep_largest, min_fraction, min_triangles, vertices is not None)
    if vertices is None:
        raise ValueError(f"{who}: vertices is None (compaction needs the [V,3] coordinates)")
    V = check_mesh(who, triangles, None, vertices)
    attributes = check_attributes(who, attributes, V)
    dev = native.same_device(triangles, vertices, *attributes.values())
    comp, tri, vts, ws = _components(who, triangles, V, vertices)
    n_comp, T = comp["n_components"], tri.shape[0]
    measure = comp["area"] if by == "area" else comp["triangles"]
    keep = select_components(measure, comp["triangles"], keep_largest, min_fraction, min_triangles)
    keep8 = keep.to(torch.uint8)
    lib = native.load()
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    with native.on_device(dev) as stream:
        native.check(lib.rnb_mesh_compact_count(native.ptr(tri), T, V, native.ptr(comp["labels"]), native.ptr(keep8), n_comp,
                                                native.ptr(ws), ws.numel(), native.ptr(counts), stream))
    counts[2] = keep.sum()
    nv, nt, n_kept = (int(c) for c in counts.cpu())
    v_out = torch.empty(nv, 3, dtype=torch.float64, device=dev) if vts is not None else None
    t_out = torch.empty(nt, 3, dtype=torch.int32, device=dev)
    index = torch.empty(nv, dtype=torch.int64, device=dev)
    with native.on_device(dev) as stream:
        native.check(lib.rnb_mesh_compact_emit(native.ptr(tri), T, native.ptr(vts), V, native.ptr(comp["labels"]),
                                               native.ptr(keep8), n_comp, native.ptr(ws), ws.numel(), nv, nt,
                                               native.ptr(v_out), native.ptr(t_out), native.ptr(index), stream))
    ids = torch.arange(n_comp, dtype=torch.int64, device=dev)
    kept = torch.sort(torch.where(keep, ids, torch.full_like(ids, n_comp))).values[:n_kept]
    info = {"n_components": n_comp, "by": by, "kept": kept, "measure": measure, "measure_kept": measure[kept],
            "n_vertices": (V, nv), "n_triangles": (T, nt)}
    return {"vertices": v_out, "triangles": t_out,
            "attributes": {k: a.index_select(0, index) for k, a in attributes.items()},
            "vertex_index": index, "info": info}


@torch.no_grad()
def compact_triangles(vertices, triangles, keep, attributes=None):
    """Keeps the triangles a per-triangle mask selects, and the vertices they name, on the device.
    vertices [V,3] float64, triangles [T,3] int32, `keep` [T] bool or uint8 (non-zero = keep) — device tensors.  A
    triangle is kept when `keep` says so and its three indices lie in [0, V) (one that does not is dropped, no address is
    formed from it); a vertex when a kept triangle names it.  Compaction is stable, as `clean_mesh`'s.
    Returns a dict shaped like `clean_mesh`'s: `vertices` [V',3], `triangles` [T',3] (remapped), `attributes` (per-vertex
    device tensors [V, ...] gathered with the same map), `vertex_index` [V'] int64 and `triangle_index` [T'] int64 (the
    old index of every kept vertex / triangle), `info`: `n_vertices` / `n_triangles` as (before, after).
    ValueError for wrong shapes / dtypes; RuntimeError for CPU tensors.  One host synchronisation (V' and T')."""
    who = "compact_triangles"
    if vertices is None:
        raise ValueError(f"{who}: vertices is None (compaction needs the [V,3] coordinates)")
    V = check_mesh(who, triangles, None, vertices)
    T = triangles.shape[0]
    if not isinstance(keep, torch.Tensor) or keep.dim() != 1 or keep.shape[0] != T or keep.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{who}: keep must be a [T] bool or uint8 tensor with T = {T}, got "
                         f"{(tuple(keep.shape), keep.dtype) if isinstance(keep, torch.Tensor) else type(keep).__name__}")
    attributes = check_attributes(who, attributes, V)
    dev = native.gpu_device(triangles, vertices, keep, *attributes.values())
    lib = native.load()
    tri, vts = triangles.detach().contiguous(), vertices.detach().contiguous()
    keep8 = keep.detach().to(torch.uint8).contiguous()
    ws = native.workspace("mesh_clean", dev, V, T)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    with native.on_device(dev) as stream:
        native.check(lib.rnb_mesh_compact_triangles_count(native.ptr(tri), T, V, native.ptr(keep8), native.ptr(ws), ws.numel(),
                                                          native.ptr(counts), stream))
    nv, nt = (int(c) for c in counts.cpu())
    v_out = torch.empty(nv, 3, dtype=torch.float64, device=dev)
    t_out = torch.empty(nt, 3, dtype=torch.int32, device=dev)
    v_index = torch.empty(nv, dtype=torch.int64, device=dev)
    t_index = torch.empty(nt, dtype=torch.int64, device=dev)
    with native.on_device(dev) as stream:
        native.check(lib.rnb_mesh_compact_triangles_emit(native.ptr(tri), T, native.ptr(vts), V, native.ptr(keep8), native.ptr(ws),
                                                         ws.numel(), nv, nt, native.ptr(v_out), native.ptr(t_out),
                                                         native.ptr(v_index), native.ptr(t_index), stream))
    return {"vertices": v_out, "triangles": t_out,
            "attributes": {k: a.index_select(0, v_index) for k, a in attributes.items()},
            "vertex_index": v_index, "triangle_index": t_index,
            "info": {"n_vertices": (V, nv), "n_triangles": (T, nt)}}
