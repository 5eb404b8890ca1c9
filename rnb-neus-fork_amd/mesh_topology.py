"""Mesh topology audit on the device: edges and how often each is used in either direction, boundary / manifold / flipped /
non-manifold edges, boundary components (holes), and per connected component the Euler characteristic, genus, closedness
and signed volume (csrc/mesh_topology.hip through `rnb_mesh_topology_*`, include/rnbneus.h, which has the definitions op
for op).  What culling, clustering and a surface that leaves the box did to the connectivity of a mesh, on the arrays the
other mesh tools leave on the GPU; there is no CPU path.

Edge-manifoldness is what is reported: a vertex where two fans touch (a "bow-tie") is not detected, and duplicate triangles
show only through their edges.

The package exports the function under the module's name: `rnb_neus_fork_amd.mesh_topology` is `mesh_topology()`, and
`watertight` stands next to it."""
from __future__ import annotations

import torch

from . import native
from .mesh_args import check_mesh

# bits of `triangle_flags` / `vertex_flags` (include/rnbneus.h)
BOUNDARY, FLIPPED, NONMANIFOLD = 1, 2, 4
TRIANGLE_DEGENERATE, TRIANGLE_INVALID = 8, 16
VERTEX_UNUSED = 8


@torch.no_grad()
def mesh_topology(triangles, n_vertices=None, vertices=None, *, edges=False, boundary=True, components=True):
    """The topology report of a triangle mesh, on the device.
    triangles [T,3] int32; `n_vertices` = V, or `vertices` [V,3] float64 (then the signed volume comes too).
    A triangle with an index outside [0, V) is INVALID (skipped: no address is formed from it), a valid one with two equal
    indices DEGENERATE; the others are proper and have the half-edges (a,b), (b,c), (c,a).  An edge is a BOUNDARY edge
    when one half-edge uses it, MANIFOLD when one uses it in each direction, FLIPPED when two use it in the same direction,
    NON-MANIFOLD when three or more do.
    Returns a dict.  Python ints: `n_edges`, `n_boundary`, `n_manifold`, `n_flipped`, `n_nonmanifold`, `n_degenerate`,
    `n_invalid`.  Device tensors: `triangle_flags` [T] uint8 (1 boundary, 2 flipped, 4 non-manifold edge; 8 degenerate, 16
    invalid), `vertex_flags` [V] uint8 (1, 2, 4 as before; 8 = named by no proper triangle).
    `boundary`: `boundary_labels` [V] int32 (boundary component of every vertex, numbered by smallest vertex, -1 off the
    boundary), `boundary_degree` [V] int32 (boundary edges at the vertex), `n_boundary_components`, `boundary_simple` (every
    boundary vertex lies on exactly two boundary edges: each boundary component is one closed loop, one hole).
    `edges`: `edges` [E,2] int32 (min, max), `edge_use` [E,2] int32 (forward, backward uses), `edge_triangle` [E] int32, in
    increasing order of each edge's first half-edge 3t + k.
    `components`: under the key `components` a dict with `labels` [V] int32 and `n_components` of `mesh_components` and
    per-component tensors `edges` [C,4] int64 (boundary, manifold, flipped, non-manifold), `triangles` (proper),
    `degenerate`, `holes` (boundary components; -1 with boundary=False), `vertices` (named by a proper triangle), `euler` =
    vertices - edges + triangles, `closed` (bool: no boundary, flipped or non-manifold edge, no degenerate triangle, and no
    invalid triangle in the mesh), `genus` (int64: (2 - euler - holes) / 2 for a component with only manifold and boundary
    edges, a simple boundary and no degenerate triangle; -1 where that is undefined) and, with `vertices`, `volume` [C]
    float64: the signed volume, bit-reproducible from run to run — the enclosed volume only for a closed, consistently
    oriented component, its sign the orientation; NaN when a non-finite corner reaches a proper triangle.
    ValueError for wrong shapes / dtypes; RuntimeError for CPU tensors.  One host synchronisation.  Never collective under
    `set_data_parallel`."""
    who = "mesh_topology"
    V = check_mesh(who, triangles, n_vertices, vertices)
    dev = native.gpu_device(triangles, vertices)
    lib = native.load()
    tri = triangles.detach().contiguous()
    vts = vertices.detach().contiguous() if vertices is not None else None
    T = tri.shape[0]
    ws = native.workspace("mesh_topology", dev, V, T)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    tri_flags = torch.empty(T, dtype=torch.uint8, device=dev)
    vert_flags = torch.empty(V, dtype=torch.uint8, device=dev)
    b_labels = torch.empty(V, dtype=torch.int32, device=dev) if boundary else None
    b_degree = torch.empty(V, dtype=torch.int32, device=dev) if boundary else None
    with native.on_device(dev) as stream:
        native.check(lib.rnb_mesh_topology_count(native.ptr(tri), T, V, native.ptr(ws), ws.numel(), native.ptr(counts),
                                                 native.ptr(tri_flags), native.ptr(vert_flags), native.ptr(b_labels),
                                                 native.ptr(b_degree), stream))
    head = [counts]
    if boundary:
        off_loop = (b_labels >= 0) & (b_degree != 2)        # boundary vertices that are not on exactly two boundary edges
        head.append(off_loop.sum().reshape(1))
    if components:
        labels = torch.empty(V, dtype=torch.int32, device=dev)
        ccounts = torch.empty(2, dtype=torch.int64, device=dev)
        cws = native.workspace("mesh_clean", dev, V, T)
        with native.on_device(dev) as stream:
            native.check(lib.rnb_mesh_components(native.ptr(tri), T, V, native.ptr(cws), cws.numel(), native.ptr(labels),
                                                 native.ptr(ccounts), stream))
        head.append(ccounts[:1])
    host = [int(c) for c in torch.cat(head).cpu()]          # the one synchronisation
    if host[0] < 0:
        raise native.NativeError(f"{who}: the edge table filled up (a fault of its sizing)")
    names = ("n_edges", "n_boundary", "n_manifold", "n_flipped", "n_nonmanifold", "n_degenerate", "n_invalid")
    out = dict(zip(names, host[:7]))
    out["triangle_flags"], out["vertex_flags"] = tri_flags, vert_flags
    if boundary:
        out.update(boundary_labels=b_labels, boundary_degree=b_degree,
                   n_boundary_components=host[7] if V > 0 else 0,      # (V = 0: the two arrays are empty, NULL to the library)
                   boundary_simple=host[8] == 0)
    if edges:
        E = host[0]
        out["edges"] = torch.empty(E, 2, dtype=torch.int32, device=dev)
        out["edge_use"] = torch.empty(E, 2, dtype=torch.int32, device=dev)
        out["edge_triangle"] = torch.empty(E, dtype=torch.int32, device=dev)
        with native.on_device(dev) as stream:
            native.check(lib.rnb_mesh_topology_emit(native.ptr(tri), T, V, native.ptr(ws), ws.numel(), E, native.ptr(out["edges"]),
                                                    native.ptr(out["edge_use"]), native.ptr(out["edge_triangle"]), stream))
    if components:
        n_comp = host[-1]
        table = torch.empty(n_comp, 8, dtype=torch.int64, device=dev)
        volume = torch.empty(n_comp, dtype=torch.float64, device=dev) if vts is not None else None
        with native.on_device(dev) as stream:
            native.check(lib.rnb_mesh_topology_components(native.ptr(tri), T, native.ptr(vts), V, native.ptr(labels), n_comp,
                                                          native.ptr(ws), ws.numel(), native.ptr(table), native.ptr(volume),
                                                          stream))
        comp = _derive(table, out["n_invalid"], labels, off_loop if boundary else None)
        comp.update(labels=labels, n_components=n_comp)
        if volume is not None:
            comp["volume"] = volume
        out["components"] = comp
    return out


def _derive(table, n_invalid, labels, off_loop):
    """euler, closed and genus from the [C,8] table of rnb_mesh_topology_components (device tensors, no synchronisation);
    `off_loop` [V] bool: boundary vertices off a simple loop, None when no boundary component was made"""
    e = table[:, :4].clone(memory_format=torch.contiguous_format)        # (columns as tensors of their own, unit stride)
    t, deg, holes, verts = (table[:, j].clone(memory_format=torch.contiguous_format) for j in range(4, 8))
    euler = verts - e.sum(dim=1) + t
    clean = (e[:, 2] == 0) & (e[:, 3] == 0) & (deg == 0)
    closed = clean & (e[:, 0] == 0) & (n_invalid == 0)
    genus = torch.full_like(euler, -1)
    if off_loop is not None and table.shape[0] > 0:
        tangled = torch.zeros_like(euler)                   # per component: boundary vertices off a simple loop (a boundary
        tangled.index_add_(0, labels.clamp(min=0).long(), off_loop.long())   # vertex is on a proper triangle: labelled)
        g2 = 2 - euler - holes
        ok = clean & (tangled == 0) & (g2 >= 0) & (g2 % 2 == 0)
        genus = torch.where(ok, g2 // 2, genus)
    return {"edges": e, "triangles": t, "degenerate": deg, "holes": holes, "vertices": verts, "euler": euler,
            "closed": closed, "genus": genus}


def watertight(report) -> bool:
    """True when the mesh of a `mesh_topology` report (made with components=True) has no invalid triangle and every
    component is closed: only manifold edges, consistently oriented, no degenerate triangle.  One host read."""
    if "components" not in report:
        raise ValueError("watertight: the report has no per-component part (mesh_topology(..., components=True))")
    return report["n_invalid"] == 0 and bool(report["components"]["closed"].all())
