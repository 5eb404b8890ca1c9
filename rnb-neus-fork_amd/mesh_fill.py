"""Mesh hole filling on the device: the boundary components of `mesh_topology` as ordered polygons, and a fan of triangles
around the centroid of every loop that can be walked (csrc/mesh_fill.hip through `rnb_mesh_loops_*` / `rnb_mesh_fill_emit`,
include/rnbneus.h, which has the definitions op for op).  What closes the holes that culling, a surface leaving the box, the
sparse grid and clustering open, on the arrays the other mesh tools leave on the GPU; there is no CPU path.

A loop is SIMPLE when it is one closed polygon, TANGLED where two holes touch (a vertex on more than two boundary edges) and
MISORIENTED where the surface changes orientation along the hole; only SIMPLE loops are walked and filled.  The cap is a
centroid fan: right for the small, roughly flat holes these tools open, and a closed but crude surface over a large or
strongly curved one (`max_edges` leaves those open)."""
from __future__ import annotations

import numbers

import torch

from . import native
from .mesh_args import check_attributes, check_mesh

SIMPLE, TANGLED, MISORIENTED = 0, 1, 2
# what the renderer's `fill=` may hold: the keywords of `fill_holes` that `check_arguments` checks
FILL_KEYWORDS = ("max_edges",)
_COUNTS = ("n_loops", "n_boundary_vertices", "n_filled", "n_new_triangles", "n_tangled", "n_misoriented", "n_too_long",
           "longest_filled", "longest_simple", "n_unwalked", "error")


def check_arguments(who, max_edges=None):
    """ValueError for a `max_edges` that is not None or an integer >= 3 (`fill_holes`, the renderer's `fill=`); the value
    the library takes (-1: no limit)"""
    if max_edges is None:
        return -1
    if isinstance(max_edges, bool) or not isinstance(max_edges, numbers.Integral) or int(max_edges) < 3:
        raise ValueError(f"{who}: max_edges must be an integer >= 3 (a loop has at least three edges), not {max_edges!r}")
    return min(int(max_edges), 2 ** 31 - 1)


class _Loops:
    """The loops of one mesh: the audit's count and the loop count enqueued, one host read, then the emit"""

    def __init__(self, who, tri, V, max_edges):
        self.who, self.tri, self.V, self.T = who, tri, V, tri.shape[0]
        self.dev, self.lib, self.max_edges = tri.device, native.load(), max_edges
        V, T, dev, lib = self.V, self.T, self.dev, self.lib
        tws = native.workspace("mesh_topology", dev, V, T)
        self.ws = native.workspace("mesh_fill", dev, V, T)
        tcounts = torch.empty(8, dtype=torch.int64, device=dev)
        counts = torch.empty(16, dtype=torch.int64, device=dev)
        tri_flags = torch.empty(T, dtype=torch.uint8, device=dev)
        vert_flags = torch.empty(V, dtype=torch.uint8, device=dev)
        self.labels = torch.empty(V, dtype=torch.int32, device=dev)
        degree = torch.empty(V, dtype=torch.int32, device=dev)
        with native.on_device(dev) as stream:
            native.check(lib.rnb_mesh_topology_count(native.ptr(tri), T, V, native.ptr(tws), tws.numel(), native.ptr(tcounts),
                                                     native.ptr(tri_flags), native.ptr(vert_flags), native.ptr(self.labels),
                                                     native.ptr(degree), stream))
            native.check(lib.rnb_mesh_loops_count(T, V, native.ptr(tws), tws.numel(), native.ptr(self.labels), native.ptr(degree),
                                                  max_edges, native.ptr(self.ws), self.ws.numel(), native.ptr(counts), stream))
        host = [int(c) for c in torch.cat([tcounts[:1], counts]).cpu()]          # the one synchronisation
        self.c = dict(zip(_COUNTS, host[1:]))
        if host[0] < 0 or self.c["error"] != 0:
            raise native.NativeError(f"{who}: the edge table filled up or a value left its range (a fault of the sizing)")
        self.L, self.B = self.c["n_loops"], self.c["n_boundary_vertices"]

    def emit(self):
        L, B, dev = self.L, self.B, self.dev
        self.offsets = torch.empty(L + 1, dtype=torch.int64, device=dev)
        self.loop_vertices = torch.empty(B, dtype=torch.int32, device=dev)
        self.status = torch.empty(L, dtype=torch.uint8, device=dev)
        self.edges = torch.empty(L, dtype=torch.int32, device=dev)
        with native.on_device(dev) as stream:
            native.check(self.lib.rnb_mesh_loops_emit(self.T, self.V, native.ptr(self.labels), native.ptr(self.ws), self.ws.numel(),
                                                      L, B, self.c["longest_simple"], self.c["n_unwalked"], native.ptr(self.offsets),
                                                      native.ptr(self.loop_vertices), native.ptr(self.status),
                                                      native.ptr(self.edges), stream))

    def mean(self, values):
        """[L,C] per-loop means of values [V,C] float64 / float32"""
        C = values.shape[1]
        out = torch.empty(self.L, C, dtype=values.dtype, device=self.dev)
        with native.on_device(self.dev) as stream:
            native.check(self.lib.rnb_mesh_loops_mean(native.ptr(values), 0 if values.dtype == torch.float64 else 1, self.V, C,
                                                      native.ptr(self.offsets), native.ptr(self.loop_vertices), self.L, self.B,
                                                      native.ptr(self.ws), self.ws.numel(), native.ptr(out), stream))
        return out


@torch.no_grad()
def boundary_loops(triangles, n_vertices=None, vertices=None):
    """The boundary of a triangle mesh as ordered loops, on the device.
    triangles [T,3] int32; `n_vertices` = V, or `vertices` [V,3] float64 (then the centroids come too).  The loops are the
    boundary components of `mesh_topology`, in its numbering (by smallest vertex).
    Returns a dict: `n_loops` (Python int); `loop_offsets` [L+1] int64 and `loop_vertices` [B] int32, the loops in CSR form —
    a SIMPLE loop starts at its smallest vertex and follows the boundary half-edges (the direction of the triangle that
    owns each edge), a loop of another status lists its vertices in increasing index; `loop_status` [L] uint8 (0 SIMPLE,
    1 TANGLED, 2 MISORIENTED); `loop_edges` [L] int32 (boundary edges of the loop); with `vertices`, `loop_centroid` [L,3]
    float64, the mean of the loop's vertex positions, bit-equal from run to run (NaN where a position is not finite).
    ValueError for wrong shapes / dtypes; RuntimeError for CPU tensors.  One host synchronisation.  Never collective under
    `set_data_parallel`."""
    who = "boundary_loops"
    V = check_mesh(who, triangles, n_vertices, vertices)
    native.gpu_device(triangles, vertices)
    loops = _Loops(who, triangles.detach().contiguous(), V, -1)
    loops.emit()
    out = {"n_loops": loops.L, "loop_offsets": loops.offsets, "loop_vertices": loops.loop_vertices,
           "loop_status": loops.status, "loop_edges": loops.edges}
    if vertices is not None:
        out["loop_centroid"] = loops.mean(vertices.detach().contiguous())
    return out


@torch.no_grad()
def fill_holes(vertices, triangles, *, max_edges=None, attributes=None):
    """Closes the holes of a mesh with centroid fans, on the device.
    vertices [V,3] float64, triangles [T,3] int32 — the tensors the other mesh tools return.  A loop of `boundary_loops` is
    filled when it is SIMPLE and has at most `max_edges` edges (an integer >= 3; None: no limit).  The filled loops are
    ranked r = 0 .. F-1 in loop order; loop r adds the vertex V + r at its centroid and, for its vertices w[0..n), the
    triangles (w[j+1 mod n], w[j], V + r), j = 0 .. n-1, appended in that order loop after loop: the cap uses every rim edge
    against its one existing use and so inherits the surface's orientation.  The old vertices and triangles come first, bit
    for bit (invalid and degenerate triangles and unreferenced vertices included).
    `attributes`: dict of per-vertex float32 device tensors [V, ...]; a new vertex gets the mean of its loop's rows (an exact
    integer sum, divided in fp64, rounded once to float32).
    Returns a dict: `vertices` [V+F,3] float64, `triangles` [T+N,3] int32, `attributes`, `filled` [F] int32 (the loop of
    every new vertex) and `info`, Python ints: `n_loops`, `n_filled`, `n_tangled`, `n_misoriented`, `n_too_long`,
    `n_new_triangles`, `longest_filled`.  With no loop to fill the input tensors themselves come back.
    ValueError for wrong shapes / dtypes and for max_edges < 3; RuntimeError for CPU tensors.  One host synchronisation.
    Never collective under `set_data_parallel`."""
    who = "fill_holes"
    limit = check_arguments(who, max_edges)
    if vertices is None:
        raise ValueError(f"{who}: vertices is None")
    V = check_mesh(who, triangles, None, vertices)
    attributes = check_attributes(who, attributes, V)
    for name, a in attributes.items():
        if a.dtype != torch.float32:
            raise ValueError(f"{who}: attribute {name!r} must be float32 (a mean is taken), not {a.dtype}")
    dev = native.gpu_device(triangles, vertices, *attributes.values())
    tri, vts = triangles.detach().contiguous(), vertices.detach().contiguous()
    loops = _Loops(who, tri, V, limit)
    c, T = loops.c, tri.shape[0]
    F, N = c["n_filled"], c["n_new_triangles"]
    info = {k: c[k] for k in ("n_loops", "n_filled", "n_tangled", "n_misoriented", "n_too_long", "n_new_triangles",
                              "longest_filled")}
    filled = torch.empty(F, dtype=torch.int32, device=dev)
    if F == 0:
        return {"vertices": vertices, "triangles": triangles, "attributes": attributes, "filled": filled, "info": info}
    if V + F > 2 ** 31 - 1 or T + N > 2 ** 31 - 1:
        raise ValueError(f"{who}: the filled mesh would have {V + F} vertices / {T + N} triangles, outside [0, 2^31 - 1]")
    loops.emit()
    centroid = loops.mean(vts)
    v_out = torch.empty(V + F, 3, dtype=torch.float64, device=dev)
    t_out = torch.empty(T + N, 3, dtype=torch.int32, device=dev)
    with native.on_device(dev) as stream:
        native.check(loops.lib.rnb_mesh_fill_emit(native.ptr(vts), V, native.ptr(tri), T, native.ptr(loops.offsets),
                                                  native.ptr(loops.loop_vertices), native.ptr(loops.status), native.ptr(centroid),
                                                  loops.L, loops.B, limit, native.ptr(loops.ws), loops.ws.numel(), F, N,
                                                  native.ptr(v_out), native.ptr(t_out), native.ptr(filled), stream))
    a_out = {}
    for name, a in attributes.items():
        flat = a.detach().reshape(V, -1).contiguous()
        rows = loops.mean(flat).index_select(0, filled.long())
        a_out[name] = torch.cat([flat, rows]).reshape((V + F,) + tuple(a.shape[1:]))
    return {"vertices": v_out, "triangles": t_out, "attributes": a_out, "filled": filled, "info": info}
