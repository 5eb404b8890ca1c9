"""numpy reference of the hole filling (rnb_neus_fork_amd.mesh_fill; the definitions of include/rnbneus.h "Mesh hole
filling"): the boundary half-edges from a dict of edges, the loops — the boundary components of
tests/mesh_topology_ref.py, in its numbering — by walking from the smallest vertex one half-edge at a time, their statuses,
their centroids by math.fsum / n, and the filled mesh in exactly the order the header states.  No device.  A helper, not a
test module; the shapes the host and the GPU tests share are built here too."""
import math

import numpy as np

from tests import mesh_large_shapes as LS
from tests import mesh_topology_ref as M

SIMPLE, TANGLED, MISORIENTED = 0, 1, 2
INFO_KEYS = ("n_loops", "n_filled", "n_tangled", "n_misoriented", "n_too_long", "n_new_triangles", "longest_filled")


def boundary_half_edges(triangles, V):
    """[(p, q)]: the half-edges of proper triangles whose undirected edge no other half-edge uses, in half-edge order"""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    _, _, proper = M.triangle_classes(t, V)
    uses = {}
    for a, b, c in t[proper].tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            uses.setdefault((min(p, q), max(p, q)), []).append((p, q))
    return [u[0] for u in uses.values() if len(u) == 1]


def mean_rows(values, members):
    """per column math.fsum over the rows `members` of `values`, divided by their number (NaN where a value is not finite)"""
    x = np.asarray(values)[members].astype(np.float64)
    out = np.empty(x.shape[1])
    for c in range(x.shape[1]):
        out[c] = math.fsum(x[:, c].tolist()) / len(members) if np.isfinite(x[:, c]).all() else np.nan
    return out


def loops(triangles, V, vertices=None):
    """dict: n_loops, loop_offsets int64 [L+1], loop_vertices int32 [B], loop_status uint8 [L], loop_edges int32 [L] and, with
    vertices, loop_centroid float64 [L,3]"""
    top = M.topology(triangles, V)
    labels, degree = top["boundary_labels"], top["boundary_degree"]
    L = int(top["counts"][7])
    nxt, n_out, n_in = {}, np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int64)
    for p, q in boundary_half_edges(triangles, V):
        nxt[p] = q
        n_out[p] += 1
        n_in[q] += 1
    order = np.argsort(labels, kind="stable")
    order = order[labels[order] >= 0]                        # the boundary vertices by (loop, index)
    starts = np.searchsorted(labels[order], np.arange(L + 1))
    status, edges, listed = np.zeros(L, dtype=np.uint8), np.zeros(L, dtype=np.int32), []
    for l in range(L):
        members = order[starts[l]:starts[l + 1]]
        edges[l] = int(degree[members].sum()) // 2
        if (degree[members] != 2).any():
            status[l] = TANGLED
        elif (n_out[members] != 1).any() or (n_in[members] != 1).any():
            status[l] = MISORIENTED
        if status[l] == SIMPLE:
            walk = [int(members[0])]
            while nxt[walk[-1]] != walk[0]:
                walk.append(nxt[walk[-1]])
                assert len(walk) <= len(members), "a SIMPLE loop is one cycle"
            assert len(walk) == len(members) and sorted(walk) == members.tolist()
            members = np.array(walk, dtype=np.int64)
        listed.append(members)
    out = {"n_loops": L, "loop_offsets": starts.astype(np.int64),
           "loop_vertices": (np.concatenate(listed) if listed else np.zeros(0)).astype(np.int32),
           "loop_status": status, "loop_edges": edges}
    if vertices is not None:
        out["loop_centroid"] = np.array([mean_rows(vertices, m) for m in listed], dtype=np.float64).reshape(L, 3)
    out["_members"] = listed
    return out


def fill(vertices, triangles, max_edges=None, attributes=None):
    """dict: vertices [V+F,3], triangles int32 [T+N,3], attributes (float32 [V+F,C] for a float32 [V,C]), filled int32 [F],
    info, and `loops` (the dict of `loops`)"""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    V = len(v)
    lp = loops(t, V, v)
    st, members = lp["loop_status"], lp["_members"]
    simple = [l for l in range(lp["n_loops"]) if st[l] == SIMPLE]
    filled = [l for l in simple if max_edges is None or len(members[l]) <= max_edges]
    new_v, new_t = [], []
    for r, l in enumerate(filled):
        w = members[l]
        new_v.append(lp["loop_centroid"][l])
        new_t += [[int(w[(j + 1) % len(w)]), int(w[j]), V + r] for j in range(len(w))]
    out = {"vertices": np.concatenate([v, np.array(new_v, dtype=np.float64).reshape(-1, 3)]),
           "triangles": np.concatenate([t, np.array(new_t, dtype=np.int32).reshape(-1, 3)]),
           "filled": np.array(filled, dtype=np.int32), "loops": lp,
           "info": {"n_loops": lp["n_loops"], "n_filled": len(filled), "n_tangled": int((st == TANGLED).sum()),
                    "n_misoriented": int((st == MISORIENTED).sum()), "n_too_long": len(simple) - len(filled),
                    "n_new_triangles": len(new_t), "longest_filled": max([len(members[l]) for l in filled], default=0)}}
    if attributes is not None:
        a = np.asarray(attributes, dtype=np.float32)
        rows = np.array([mean_rows(a, members[l]) for l in filled], dtype=np.float64).reshape(-1, a.shape[1])
        out["attributes"] = np.concatenate([a, rows.astype(np.float32)])
        out["attribute_means"] = rows
    return out


def mean_bound(values, members):
    """per column n 2^-52 mean|x|: a sum in any order errs by at most (n - 1) 2^-53 sum|x|, the division adds one rounding,
    the factor 2 is for the second-order terms"""
    x = np.abs(np.asarray(values)[members].astype(np.float64))
    return len(members) * 2.0 ** -52 * x.mean(axis=0)


def euler_sum(report):
    return int(report["euler"].sum())


# ---- shapes -------------------------------------------------------------------------------------------------------------

def tube(n, rings=3):
    """an open cylinder of radius 1: `rings` rings of n vertices at z = 0, 1, ..; vertex ring * n + i; 2 n (rings - 1)
    triangles, outward.  Two n-edge loops; filled, its volume is (rings - 1) x the area of the n-gon"""
    w = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([np.stack([np.cos(w), np.sin(w), np.full(n, float(r))], axis=1) for r in range(rings)])
    i = np.arange(n)
    t = []
    for r in range(rings - 1):
        a, b, c, d = r * n + i, r * n + (i + 1) % n, (r + 1) * n + (i + 1) % n, (r + 1) * n + i
        t.append(np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], axis=1).reshape(-1, 3))
    return np.ascontiguousarray(v), np.ascontiguousarray(np.concatenate(t).astype(np.int32))


def ngon_area(n):
    return 0.5 * n * math.sin(2 * math.pi / n)


def inside_out(mesh):
    v, t = mesh
    return v, np.ascontiguousarray(t[:, ::-1])


def open_tetrahedron():
    """the tetrahedron less its last face: one 3-edge loop; filled, volume 1/6"""
    v, t = M.tetrahedron()
    return v, np.ascontiguousarray(t[:-1])


def punched_sheet(m, k, q):
    """`mesh_large_shapes.sheet(m, k)` with every q-th quad removed (quad j = row * k + column, j % q == 0).  No two removed
    quads touch when q divides none of 1, k - 1, k, k + 1: every removed interior quad is a 4-edge hole of its own"""
    assert all(d % q for d in (1, k - 1, k, k + 1)), "removed quads would touch"
    v, t = LS.sheet(m, k)
    keep = np.repeat(np.arange(m * k) % q != 0, 2)
    return v, np.ascontiguousarray(t[keep])


def punched_holes(m, k, q):
    """the number of removed quads of `punched_sheet` that lie inside the sheet (not on its rim)"""
    j = np.arange(m * k)
    r, c = j // k, j % k
    return int(((j % q == 0) & (r > 0) & (r < m - 1) & (c > 0) & (c < k - 1)).sum())
