"""numpy reference of the mesh topology audit (rnb_neus_fork_amd.mesh_topology; the definitions of include/rnbneus.h "Mesh
topology audit"), stated twice: `topology` vectorised (edge keys, np.unique with the first index, np.add.at, components by
minimum-label propagation) and `topology_brute` as a plain dict-of-edges loop with a sequential union-find, for small
meshes.  The volume term is evaluated in the kernel's operation order, one rounding per operation, and summed per
component with math.fsum.  A helper, not a test module; the shapes the host and the GPU tests share are built here too."""
import math

import numpy as np

BOUNDARY, FLIPPED, NONMANIFOLD, DEGENERATE, INVALID, UNUSED = 1, 2, 4, 8, 16, 8
INT_KEYS = ("counts", "triangle_flags", "vertex_flags", "boundary_labels", "boundary_degree", "edges", "edge_use",
            "edge_triangle", "labels", "table", "euler", "closed", "genus")


def triangle_classes(triangles, V):
    """(invalid, degenerate, proper) [T] bool"""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    invalid = ((t < 0) | (t >= V)).any(axis=1)
    degenerate = ~invalid & ((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2]))
    return invalid, degenerate, ~invalid & ~degenerate


def roots(V, a, b):
    """root[v] = the smallest vertex of v's class under the transitive closure of the pairs (a[i], b[i])"""
    root = np.arange(V, dtype=np.int64)
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    while True:
        ra, rb = root[a], root[b]
        m = np.minimum(ra, rb)
        new = root.copy()
        np.minimum.at(new, ra, m)
        np.minimum.at(new, rb, m)
        while True:
            nn = new[new]
            if np.array_equal(nn, new):
                break
            new = nn
        if np.array_equal(new, root):
            return root
        root = new


def dense_labels(root, member):
    """classes numbered in increasing order of their smallest member; -1 where `member` is False; and their number"""
    V = len(root)
    is_root = member & (root == np.arange(V))
    rank = np.cumsum(is_root) - 1
    return np.where(member, rank[root] if V else root, -1).astype(np.int32), int(is_root.sum())


def edge_class(nf, nb):
    n = nf + nb
    return np.where(n == 1, BOUNDARY, np.where(n == 2, np.where(nf == 1, 0, FLIPPED), NONMANIFOLD))


def volume_terms(vertices, t):
    """((x0 cx + y0 cy) + z0 cz) / 6 per triangle, every operation rounded on its own, and whether the nine coordinates and
    the term are finite"""
    p = np.asarray(vertices, dtype=np.float64)[t]
    x0, y0, z0 = p[:, 0, 0], p[:, 0, 1], p[:, 0, 2]
    x1, y1, z1 = p[:, 1, 0], p[:, 1, 1], p[:, 1, 2]
    x2, y2, z2 = p[:, 2, 0], p[:, 2, 1], p[:, 2, 2]
    with np.errstate(all="ignore"):
        cx = y1 * z2 - z1 * y2
        cy = z1 * x2 - x1 * z2
        cz = x1 * y2 - y1 * x2
        xy = x0 * cx + y0 * cy
        d = xy + z0 * cz
        term = d / 6.0
    return term, np.isfinite(p).all(axis=(1, 2)) & np.isfinite(term)


def _derived(out, n_invalid):
    tab = out["table"]
    e, tc, deg, holes, verts = tab[:, :4], tab[:, 4], tab[:, 5], tab[:, 6], tab[:, 7]
    out["euler"] = verts - e.sum(axis=1) + tc
    clean = (e[:, 2] == 0) & (e[:, 3] == 0) & (deg == 0)
    out["closed"] = clean & (e[:, 0] == 0) & (n_invalid == 0)
    lab = out["labels"]
    off = (out["boundary_labels"] >= 0) & (out["boundary_degree"] != 2)
    tangled = np.bincount(lab[off].astype(np.int64), minlength=len(tab))
    g2 = 2 - out["euler"] - holes
    ok = clean & (tangled == 0) & (g2 >= 0) & (g2 % 2 == 0)
    out["genus"] = np.where(ok, g2 // 2, -1).astype(np.int64)


def _volume(out, vertices, t, proper):
    C = len(out["table"])
    tp = t[proper]
    term, fin = volume_terms(vertices, tp)
    comp = out["labels"][tp[:, 0]].astype(np.int64)
    vol, bound = np.zeros(C), np.zeros(C)
    for c in range(C):
        mine = comp == c
        if (mine & ~fin).any():
            vol[c] = np.nan
            continue
        x = term[mine]
        vol[c] = math.fsum(x.tolist())
        m = float(np.abs(x).max()) if len(x) else 0.0
        bound[c] = len(x) * 2.0 ** -55 * m + 2.0 ** -52 * abs(vol[c])
    out["volume"], out["volume_bound"] = vol, bound


def topology(triangles, V, vertices=None):
    """The whole report as numpy arrays (the keys of INT_KEYS, `boundary_simple`, `n_components`, and with `vertices`
    `volume` and `volume_bound` [C]: n_c 2^-55 M_c + 2^-52 |volume|)."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    V = int(V)
    invalid, degenerate, proper = triangle_classes(t, V)
    h = np.flatnonzero(np.repeat(proper, 3))                                # the half-edges, by index 3t + k
    p = t.reshape(-1)[h]
    q = np.roll(t, -1, axis=1).reshape(-1)[h]
    key = np.minimum(p, q) * 2 ** 31 + np.maximum(p, q)
    ukey, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    leader = h[first]                                                        # (np.unique: the FIRST occurrence, h ascending)
    order = np.argsort(leader, kind="stable")
    pos = np.empty(len(order), dtype=np.int64)
    pos[order] = np.arange(len(order))
    edge_of = pos[inverse.reshape(-1)]                                       # edge (in leader order) of every half-edge
    E = len(ukey)
    use = np.zeros((E, 2), dtype=np.int64)
    np.add.at(use, (edge_of, (p > q).astype(np.int64)), 1)
    edges = np.stack([ukey[order] >> 31, ukey[order] & (2 ** 31 - 1)], axis=1)
    cls = edge_class(use[:, 0], use[:, 1])
    tri_flags = np.where(invalid, INVALID, np.where(degenerate, DEGENERATE, 0)).astype(np.int64)
    np.bitwise_or.at(tri_flags, h // 3, cls[edge_of])
    vert_flags = np.zeros(V, dtype=np.int64)
    np.bitwise_or.at(vert_flags, edges[:, 0], cls)
    np.bitwise_or.at(vert_flags, edges[:, 1], cls)
    named = np.zeros(V, dtype=bool)
    named[t[proper].reshape(-1)] = True
    vert_flags[~named] |= UNUSED
    be = edges[cls == BOUNDARY]
    degree = np.bincount(be.reshape(-1), minlength=V).astype(np.int32)
    broot = roots(V, be[:, 0], be[:, 1])
    blabels, n_bc = dense_labels(broot, degree > 0)
    out = {"counts": np.array([E, (cls == BOUNDARY).sum(), (cls == 0).sum(), (cls == FLIPPED).sum(), (cls == NONMANIFOLD).sum(),
                               degenerate.sum(), invalid.sum(), n_bc], dtype=np.int64),
           "triangle_flags": tri_flags.astype(np.uint8), "vertex_flags": vert_flags.astype(np.uint8),
           "boundary_labels": blabels, "boundary_degree": degree, "boundary_simple": bool((degree[degree > 0] == 2).all()),
           "edges": edges.astype(np.int32), "edge_use": use.astype(np.int32), "edge_triangle": (leader[order] // 3).astype(np.int32)}
    # components: those of the cleanup (every valid triangle connects its corners, degenerate ones included)
    tv = t[~invalid]
    croot = roots(V, np.concatenate([tv[:, 0], tv[:, 1]]), np.concatenate([tv[:, 1], tv[:, 2]]))
    referenced = np.zeros(V, dtype=bool)
    referenced[tv.reshape(-1)] = True
    labels, C = dense_labels(croot, referenced)
    table = np.zeros((C, 8), dtype=np.int64)
    col = np.select([cls == BOUNDARY, cls == 0, cls == FLIPPED], [0, 1, 2], 3)
    np.add.at(table, (labels[edges[:, 0]].astype(np.int64), col), 1)
    table[:, 4] = np.bincount(labels[t[proper][:, 0]].astype(np.int64), minlength=C)
    table[:, 5] = np.bincount(labels[t[degenerate][:, 0]].astype(np.int64), minlength=C)
    is_broot = (degree > 0) & (broot == np.arange(V))
    table[:, 6] = np.bincount(labels[is_broot].astype(np.int64), minlength=C)
    table[:, 7] = np.bincount(labels[named].astype(np.int64), minlength=C)
    out.update(labels=labels, n_components=C, table=table)
    _derived(out, int(invalid.sum()))
    if vertices is not None:
        _volume(out, vertices, t, proper)
    return out


def topology_brute(triangles, V, vertices=None):
    """The same report by a plain loop: a dict of edges in order of first appearance, sequential union-finds."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    V, T = int(V), len(t)
    tri_flags, vert_flags = [0] * T, [UNUSED] * V
    table_of, n_deg, n_inv = {}, 0, 0                       # key -> [leader, n_fwd, n_bwd]
    for i, (a, b, c) in enumerate(t.tolist()):
        if min(a, b, c) < 0 or max(a, b, c) >= V:
            tri_flags[i], n_inv = INVALID, n_inv + 1
        elif a == b or b == c or a == c:
            tri_flags[i], n_deg = DEGENERATE, n_deg + 1
        else:
            for k, (x, y) in enumerate(((a, b), (b, c), (c, a))):
                rec = table_of.setdefault((min(x, y), max(x, y)), [3 * i + k, 0, 0])
                rec[1 if x < y else 2] += 1
                vert_flags[x] &= ~UNUSED

    def find(parent, x):
        while parent[x] != x:
            x = parent[x]
        return x

    def unite(parent, x, y):
        rx, ry = find(parent, x), find(parent, y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)

    listed = sorted(table_of.items(), key=lambda kv: kv[1][0])
    counts = [len(listed), 0, 0, 0, 0, n_deg, n_inv, 0]
    degree, bparent, cls_of = [0] * V, list(range(V)), {}
    for (x, y), (_, nf, nb) in listed:
        n = nf + nb
        cl = BOUNDARY if n == 1 else (0 if nf == 1 else FLIPPED) if n == 2 else NONMANIFOLD
        cls_of[(x, y)] = cl
        counts[{BOUNDARY: 1, 0: 2, FLIPPED: 3, NONMANIFOLD: 4}[cl]] += 1
        vert_flags[x] |= cl
        vert_flags[y] |= cl
        if cl == BOUNDARY:
            degree[x] += 1
            degree[y] += 1
            unite(bparent, x, y)
    for i, (a, b, c) in enumerate(t.tolist()):
        if tri_flags[i] == 0:
            for x, y in ((a, b), (b, c), (c, a)):
                tri_flags[i] |= cls_of[(min(x, y), max(x, y))]
    broot = np.array([find(bparent, v) for v in range(V)], dtype=np.int64)
    degree = np.array(degree, dtype=np.int32)
    blabels, counts[7] = dense_labels(broot, degree > 0)
    out = {"counts": np.array(counts, dtype=np.int64), "triangle_flags": np.array(tri_flags, dtype=np.uint8),
           "vertex_flags": np.array(vert_flags, dtype=np.uint8), "boundary_labels": blabels, "boundary_degree": degree,
           "boundary_simple": all(d in (0, 2) for d in degree.tolist()),
           "edges": np.array([k for k, _ in listed], dtype=np.int32).reshape(-1, 2),
           "edge_use": np.array([r[1:] for _, r in listed], dtype=np.int32).reshape(-1, 2),
           "edge_triangle": np.array([r[0] // 3 for _, r in listed], dtype=np.int32)}
    cparent, referenced = list(range(V)), np.zeros(V, dtype=bool)
    for i, (a, b, c) in enumerate(t.tolist()):
        if tri_flags[i] != INVALID:
            unite(cparent, a, b)
            unite(cparent, b, c)
            referenced[[a, b, c]] = True
    labels, C = dense_labels(np.array([find(cparent, v) for v in range(V)], dtype=np.int64), referenced)
    table = np.zeros((C, 8), dtype=np.int64)
    for (x, y), _ in listed:
        table[labels[x], {BOUNDARY: 0, 0: 1, FLIPPED: 2, NONMANIFOLD: 3}[cls_of[(x, y)]]] += 1
    for i, (a, b, c) in enumerate(t.tolist()):
        if tri_flags[i] != INVALID:
            table[labels[a], 5 if tri_flags[i] == DEGENERATE else 4] += 1
    for v in range(V):
        if degree[v] > 0 and broot[v] == v:
            table[labels[v], 6] += 1
        if not vert_flags[v] & UNUSED:
            table[labels[v], 7] += 1
    out.update(labels=labels, n_components=C, table=table)
    _derived(out, n_inv)
    if vertices is not None:
        _volume(out, vertices, t, np.array([f & (INVALID | DEGENERATE) == 0 for f in tri_flags], dtype=bool))
    return out


def equal(a, b):
    """the first key in which two reports differ, or None (integers and NaN positions exactly; the two formulations share the
    volume code, so volumes are compared exactly too)"""
    for k in INT_KEYS:
        if not np.array_equal(a[k], b[k]):
            return k
    if a["boundary_simple"] != b["boundary_simple"] or a["n_components"] != b["n_components"]:
        return "boundary_simple / n_components"
    if "volume" in a and not np.array_equal(a["volume"], b["volume"], equal_nan=True):
        return "volume"
    return None


# ---- shapes -------------------------------------------------------------------------------------------------------------

def _arr(v, t):
    return np.asarray(v, dtype=np.float64).reshape(-1, 3), np.asarray(t, dtype=np.int32).reshape(-1, 3)


def tetrahedron(at=(0.0, 0.0, 0.0)):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64) + np.asarray(at)
    return _arr(v, [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])           # outward: volume +1/6


def cube(open_top=False):
    v = [[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)]
    quads = [(0, 2, 3, 1), (0, 1, 5, 4), (1, 3, 7, 5), (3, 2, 6, 7), (2, 0, 4, 6)] + ([] if open_top else [(4, 5, 7, 6)])
    return _arr(v, [tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))])


def torus_grid(m, n, R=1.0, r=0.35):
    """a closed grid of m x n quads on a torus, two triangles per quad, consistently oriented: V = m n, T = 2 m n, E = 3 m n"""
    i, j = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
    u, w = 2 * np.pi * i / m, 2 * np.pi * j / n
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], axis=-1).reshape(-1, 3)
    a = (i * n + j).reshape(-1)
    b = (((i + 1) % m) * n + j).reshape(-1)
    c = (((i + 1) % m) * n + (j + 1) % n).reshape(-1)
    d = (i * n + (j + 1) % n).reshape(-1)
    return _arr(v, np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], axis=1).reshape(-1, 3))


def moebius(n=12):
    """a strip of n quads closed with a half twist: 2 rows of n vertices, the last quad joins row 0 to row 1"""
    u = 2 * np.pi * np.arange(n) / n
    v = []
    for s in (-0.3, 0.3):
        v.append(np.stack([(1 + s * np.cos(u / 2)) * np.cos(u), (1 + s * np.cos(u / 2)) * np.sin(u), s * np.sin(u / 2)], axis=1))
    t = []
    for i in range(n):
        a, b = i, n + i
        c, d = (i + 1, n + i + 1) if i + 1 < n else (n, 0)                  # the twist: top meets bottom
        t += [[a, c, d], [a, d, b]]
    return _arr(np.concatenate(v), t)


def icosphere(level=2):
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nt = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in t:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = nt
    return _arr(np.array(v), t)


def polyhedral_volume(v, t):
    """sum of det[p0 p1 p2] / 6 in extended precision (np.longdouble where the platform has it), as a float"""
    p = np.asarray(v, dtype=np.longdouble)[np.asarray(t, dtype=np.int64)]
    return float((p[:, 0] * np.cross(p[:, 1], p[:, 2])).sum() / 6)


def shared_edge_tetrahedra():
    """two tetrahedra that share the edge (0, 1) and nothing else: that edge is used four times"""
    v0, t0 = tetrahedron()
    v1 = np.array([[0, 0, 0], [1, 0, 0], [0, -1, 0], [0, 0, -1]], dtype=np.float64)
    remap = np.array([0, 1, 4, 5])
    return _arr(np.concatenate([v0, v1[2:]]), np.concatenate([t0, remap[t0]]))


def icosphere_one_reversed(level=1, which=5):
    v, t = icosphere(level)
    t = t.copy()
    t[which] = t[which][::-1]
    return v, t


def bow_tie():
    """two triangles that share only vertex 0: its boundary degree is 4"""
    return _arr([[0, 0, 0], [1, 0, 0], [1, 1, 0], [-1, 0, 0], [-1, -1, 0]], [[0, 1, 2], [0, 3, 4]])


def strip(n_triangles):
    """a zig-zag strip: triangle i = (i, i+1, i+2), alternately reversed so that the orientation is consistent"""
    k = np.arange(n_triangles)
    v = np.stack([np.arange(n_triangles + 2) // 2, np.arange(n_triangles + 2) % 2, np.zeros(n_triangles + 2)], axis=1) * 0.5
    t = np.stack([k, k + 1, k + 2], axis=1)
    t[1::2] = t[1::2][:, [1, 0, 2]]
    return _arr(v, t)


def fan(n=1000, mixed=False):
    """n triangles around the one edge (0, 1): use (n, 0), or mixed directions"""
    w = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([[[0, 0, -1], [0, 0, 1]], np.stack([np.cos(w), np.sin(w), np.zeros(n)], axis=1)])
    t = np.stack([np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64), 2 + np.arange(n)], axis=1)
    if mixed:
        t[::3] = t[::3][:, [1, 0, 2]]
    return _arr(v, t)


def degenerate_input():
    """in one mesh: a triangle (a, a, b), one with index V and one with -1, unreferenced vertices, and a duplicate of an
    existing triangle; V = 12"""
    v, t = cube(open_top=True)
    v = np.concatenate([v, [[2, 2, 2], [3, 3, 3], [4, 4, 4], [5, 5, 5]]])          # 8, 9 used below; 10, 11 unreferenced
    extra = [[8, 8, 9], [0, 1, 12], [2, -1, 3], list(t[3]), [0, 9, 8]]
    return _arr(v, np.concatenate([t, extra]))


def interleave(meshes, seed=0):
    """the meshes as ONE mesh whose vertex numbering interleaves them (a seeded permutation), triangle order shuffled too"""
    vs, ts, off = [], [], 0
    for v, t in meshes:
        vs.append(v)
        ts.append(t + off)
        off += len(v)
    v, t = np.concatenate(vs), np.concatenate(ts)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(v))                         # new index of every old vertex
    out = np.empty_like(v)
    out[perm] = v
    return _arr(out, perm[t][rng.permutation(len(t))])


def small_shapes():
    s = {"tetrahedron": tetrahedron(), "open cube": cube(open_top=True), "torus 8x6": torus_grid(8, 6), "moebius": moebius(),
         "shared edge": shared_edge_tetrahedra(), "one reversed": icosphere_one_reversed(), "bow tie": bow_tie()}
    s["all interleaved"] = interleave(list(s.values()))
    return s


def torus_with_holes(m=600, n=300, n_removed=1000, seed=11):
    v, t = torus_grid(m, n)
    keep = np.ones(len(t), dtype=bool)
    keep[np.random.default_rng(seed).choice(len(t), n_removed, replace=False)] = False
    return v, t[keep]
