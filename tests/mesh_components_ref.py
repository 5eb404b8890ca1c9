"""numpy reference of the mesh cleanup (rnb_neus_fork_amd.mesh_clean): components, statistics, selection, compaction —
the definitions of DESIGN.md "Mesh cleanup", written the plain way (a sequential union-find; no scipy).  A helper, not a
test module; the volumes the host and the GPU tests share are built here too."""
import numpy as np


def components(triangles, n_vertices):
    """labels [V] int32 (-1 = unreferenced) and C.  Two vertices are connected when a triangle names both; components
    are numbered in increasing order of their smallest vertex index."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    V = int(n_vertices)
    if t.size and (t.min() < 0 or t.max() >= V):
        raise ValueError("triangle index out of range")
    parent = list(range(V))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in t.tolist():
        for x, y in ((a, b), (b, c)):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    root = np.array([find(v) for v in range(V)], dtype=np.int64)       # the smallest vertex of the component
    referenced = np.zeros(V, dtype=bool)
    referenced[t.reshape(-1)] = True
    is_root = referenced & (root == np.arange(V))
    rank = np.cumsum(is_root) - 1
    labels = np.where(referenced, rank[root] if V else root, -1).astype(np.int32)
    return labels, int(is_root.sum())


def triangle_areas(vertices, triangles):
    p = np.asarray(vertices, dtype=np.float64)[np.asarray(triangles, dtype=np.int64)]
    return 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)


def stats(triangles, labels, n_components, vertices=None):
    """dict: triangles [C], vertices [C] int64; with coordinates area [C], bbox_min / bbox_max [C,3] float64 (a NaN
    coordinate makes the component's area and that axis of its bbox NaN)."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    C = int(n_components)
    tl = labels[t[:, 0]].astype(np.int64)
    out = {"triangles": np.bincount(tl, minlength=C).astype(np.int64),
           "vertices": np.bincount(labels[labels >= 0].astype(np.int64), minlength=C).astype(np.int64)}
    if vertices is not None:
        v = np.asarray(vertices, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            out["area"] = np.bincount(tl, weights=triangle_areas(v, t), minlength=C).astype(np.float64)
        lo, hi = np.full((C, 3), np.inf), np.full((C, 3), -np.inf)
        ref = labels >= 0
        np.minimum.at(lo, labels[ref].astype(np.int64), v[ref])
        np.maximum.at(hi, labels[ref].astype(np.int64), v[ref])
        out["bbox_min"], out["bbox_max"] = lo, hi
    return out


def area_bound(vertices, triangles, labels, n_components):
    """(n_c + 16) 2^-52 S_c per component, S_c = sum of 0.5 |e1| |e2| over its n_c triangles: n_c 2^-52 S_c covers two
    summation orders (and the device's rounding of every triangle to 2^-55 of the largest), 16 x 2^-52 S_c a few ulps of
    evaluation-order difference per triangle."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    p = np.asarray(vertices, dtype=np.float64)[t]
    s = 0.5 * np.linalg.norm(p[:, 1] - p[:, 0], axis=1) * np.linalg.norm(p[:, 2] - p[:, 0], axis=1)
    tl = labels[t[:, 0]].astype(np.int64)
    S = np.bincount(tl, weights=s, minlength=n_components)
    n = np.bincount(tl, minlength=n_components)
    return (n + 16) * 2.0 ** -52 * S


def select(measure, n_triangles, keep_largest=None, min_fraction=None, min_triangles=None):
    """keep [C] bool: the criteria given, ANDed.  keep_largest: the k largest measures, ties to the smaller id, NaN below
    every number; min_fraction: measure >= f x the largest number (NaN never passes)."""
    m = np.asarray(measure, dtype=np.float64)
    C = len(m)
    keep = np.ones(C, dtype=bool)
    if C == 0:
        return keep
    ranked = np.where(np.isnan(m), -np.inf, m)
    if keep_largest is not None:
        order = sorted(range(C), key=lambda c: (-ranked[c], c))[:int(keep_largest)]
        top = np.zeros(C, dtype=bool)
        top[order] = True
        keep &= top
    if min_fraction is not None:
        with np.errstate(invalid="ignore"):
            keep &= m >= float(min_fraction) * ranked.max()
    if min_triangles is not None:
        keep &= np.asarray(n_triangles) >= int(min_triangles)
    return keep


def compact(vertices, triangles, labels, keep):
    """Stable compaction to the kept components: (v[keep_v], newidx[t[keep_t]], old index of every kept vertex)."""
    t = np.asarray(triangles).reshape(-1, 3)
    keep_v = np.zeros(len(labels), dtype=bool)
    keep_v[labels >= 0] = keep[labels[labels >= 0]]
    keep_t = keep_v[t[:, 0]] if len(t) else np.zeros(0, dtype=bool)
    newidx = (np.cumsum(keep_v) - 1).astype(np.int32)
    return np.asarray(vertices)[keep_v], newidx[t[keep_t].astype(np.int64)].astype(np.int32).reshape(-1, 3), np.flatnonzero(keep_v)


def clean(vertices, triangles, by="area", keep_largest=None, min_fraction=None, min_triangles=None):
    """The whole of clean_mesh: (vertices', triangles', vertex_index, keep [C], stats)."""
    labels, C = components(triangles, len(vertices))
    st = stats(triangles, labels, C, vertices)
    keep = select(st[by], st["triangles"], keep_largest, min_fraction, min_triangles)
    v, t, index = compact(vertices, triangles, labels, keep)
    return v, t, index, keep, st


# ---- the volumes of the tests ---------------------------------------------------------------------------------------
A_SPHERES = (((-0.3, 0.0, 0.05), 0.45), ((0.6, 0.5, 0.4), 0.12), ((0.55, -0.6, -0.5), 0.2))


def volume_a(n=40, spheres=A_SPHERES):
    """u = -min over the spheres (tests/mc_shapes.sphere on linspace(-1, 1, n)^3, fp32): a big sphere and two floaters."""
    from tests.mc_shapes import sphere
    return -np.minimum.reduce([sphere(n, r, c) for c, r in spheres])


def noise_volume():
    """the noise volume of test_gpu_mcubes.py: seed 5, 37 x 21 x 50, walls set to 2"""
    rng = np.random.default_rng(5)
    u = rng.standard_normal((37, 21, 50)).astype(np.float32)
    u[0], u[-1], u[:, 0], u[:, -1], u[:, :, 0], u[:, :, -1] = 2, 2, 2, 2, 2, 2
    return u


# ---- small meshes that stress the union-find and the scans ----------------------------------------------------------
def renumber(vertices, triangles, perm):
    """vertex j becomes vertex perm[j]"""
    perm = np.asarray(perm, dtype=np.int64)
    v = np.empty_like(vertices)
    v[perm] = vertices
    return v, perm[np.asarray(triangles, dtype=np.int64)].astype(np.int32)


def strip(n_triangles, order):
    """a triangle strip (one component) whose vertices are numbered along it ("ascending"), against it ("descending") or
    in bit-reversed order: every hook of the union-find lands on a long chain"""
    n = n_triangles + 2
    j = np.arange(n)
    pos = np.stack([0.5 * j, (j % 2).astype(np.float64), 0.25 * np.sin(j)], axis=1)
    tri = np.stack([j[:-2], j[1:-1], j[2:]], axis=1).astype(np.int32)
    if order == "ascending":
        perm = j
    elif order == "descending":
        perm = j[::-1]
    else:
        assert order == "bitrev", order
        bits = int(np.ceil(np.log2(n)))
        rev = np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)])
        perm = np.argsort(np.argsort(rev, kind="stable"), kind="stable")
    return renumber(pos, tri, perm)


def two_fans(k=40):
    """two fans (centres 0 and k + 1) that share the one rim vertex k: one component"""
    ang = np.linspace(0.0, 1.5 * np.pi, k)
    rim1 = np.stack([np.cos(ang), np.sin(ang), np.zeros(k)], axis=1)
    rim2 = rim1[:-1] * 0.7 + np.array([0.0, -1.7, 0.3])
    v = np.concatenate([[[0.0, 0.0, 0.0]], rim1, [[0.0, -1.7, 0.3]], rim2])
    t1 = [(0, i, i + 1) for i in range(1, k)]
    c2, r2 = k + 1, list(range(k + 2, 2 * k + 1)) + [k]
    t2 = [(c2, r2[i], r2[i + 1]) for i in range(len(r2) - 1)]
    return v, np.array(t1 + t2, dtype=np.int32)


def isolated(n_triangles, seed=0):
    """n disjoint triangles of random sizes: C = T"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((3 * n_triangles, 3)) * rng.uniform(0.1, 3.0, (n_triangles, 1)).repeat(3, axis=0)
    return v, np.arange(3 * n_triangles, dtype=np.int32).reshape(-1, 3)


def degenerate():
    """duplicates, a reversed copy, (a,a,b), (a,a,a) and (a,b,b); vertex 7 is unreferenced"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 2], [3, 2, 2], [5, 5, 5], [3, 3, 2], [9, 9, 9]], dtype=np.float64)
    t = np.array([(0, 1, 2), (0, 1, 2), (2, 1, 0), (3, 3, 4), (5, 5, 5), (4, 6, 6)], dtype=np.int32)
    return v, t


def with_unreferenced(n_triangles=7):
    """disjoint triangles with unreferenced vertices at index 0, in the middle and at V - 1"""
    v, t = isolated(n_triangles, seed=1)
    gaps = np.array([0, 10, len(v) + 2])                      # positions of the unreferenced vertices in the new array
    V = len(v) + 3
    old_to_new = np.setdiff1d(np.arange(V), gaps)
    vv = np.full((V, 3), 100.0)
    vv[old_to_new] = v
    return vv, old_to_new[t].astype(np.int32)


SMALL_MESHES = {
    "strip_ascending": lambda: strip(2049, "ascending"),
    "strip_descending": lambda: strip(2049, "descending"),
    "strip_bitrev": lambda: strip(2049, "bitrev"),
    "two_fans": two_fans,
    "isolated_1": lambda: isolated(1),
    "isolated_255": lambda: isolated(255),
    "isolated_256": lambda: isolated(256),
    "isolated_257": lambda: isolated(257),
    "isolated_1025": lambda: isolated(1025),
    "degenerate": degenerate,
    "unreferenced": with_unreferenced,
}
