"""numpy reference of the mesh simplification (rnb_neus_fork_amd.mesh_simplify, csrc/mesh_simplify.hip): the definition
of include/rnbneus.h "Mesh simplification", op for op — uint64 sums, every float64 step on its own line — and a second,
independent formulation (brute force over np.unique of the cell triples, Python sets for the duplicates).  A helper, not
a test module.

Both return a dict: `vertices` [V',3], `triangles` [T',3] int32, `vertex_index` [V'] int64, `vertex_cluster` [V] int32,
`triangle_index` [T'] int64, `counts` = [V', T', degenerate, duplicate, flags, clusters] and `origin` [3]."""
import numpy as np

LIMIT = 2 ** 20
FLAG_BAD_INDEX, FLAG_BAD_VERTEX = 1, 2


def default_origin(vertices):
    """per axis the minimum over the vertices whose three coordinates are finite; zeros when there is none"""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    ok = np.isfinite(v).all(axis=1)
    return v[ok].min(axis=0) if ok.any() else np.zeros(3)


def cells(vertices, origin, h):
    """(i [V,3] int64, f [V,3] float64, usable [V] bool): u = (x - origin) / h, i = floor(u), f = u - i"""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    o = np.asarray(origin, dtype=np.float64).reshape(1, 3)
    h = np.float64(h)
    with np.errstate(all="ignore"):
        d = v - o
        u = d / h
        fl = np.floor(u)
        inside = (fl >= -float(LIMIT)) & (fl < float(LIMIT))            # false for NaN / infinite u
        usable = np.isfinite(v).all(axis=1) & inside.all(axis=1)
        f = u - fl
    i = np.where(usable[:, None], fl, 0.0).astype(np.int64)
    return i, np.where(usable[:, None], f, 0.0), usable


def _valid(triangles, V, usable):
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    in_range = ((t >= 0) & (t < V)).all(axis=1)
    safe = np.where(in_range[:, None], t, 0)
    ok_vertices = usable[safe].all(axis=1) if V else np.zeros(len(t), dtype=bool)
    valid = in_range & ok_vertices
    flags = (FLAG_BAD_INDEX if (~in_range).any() else 0) | (FLAG_BAD_VERTEX if (in_range & ~ok_vertices).any() else 0)
    return t, valid, flags


def _assemble(vertices, t, V, lead, rep, survive, counts_tail, origin):
    """the output from: lead [V] (leader of every vertex's cluster, -1 = none), rep (by leader), survive [T] bool"""
    st = t[survive]
    used = np.zeros(V, dtype=bool)
    if len(st):
        used[lead[st].reshape(-1)] = True                       # by leader
    out_leaders = np.flatnonzero(used)                          # increasing order of leader
    newidx = np.full(V, -1, dtype=np.int64)
    newidx[out_leaders] = np.arange(len(out_leaders))
    vertex_index = rep[out_leaders].astype(np.int64)
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    vertex_cluster = np.where(lead >= 0, newidx[np.maximum(lead, 0)], -1).astype(np.int32)
    triangles = newidx[lead[st]].astype(np.int32).reshape(-1, 3)
    return {"vertices": v[vertex_index].reshape(-1, 3), "triangles": triangles, "vertex_index": vertex_index,
            "vertex_cluster": vertex_cluster, "triangle_index": np.flatnonzero(survive).astype(np.int64),
            "counts": [len(out_leaders), int(survive.sum())] + counts_tail, "origin": np.asarray(origin, dtype=np.float64)}


def simplify(vertices, triangles, cell_size, origin=None):
    """The definition, op for op."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    V = len(v)
    origin = default_origin(v) if origin is None else np.asarray(origin, dtype=np.float64)
    i, f, usable = cells(v, origin, cell_size)
    t, valid, flags = _valid(triangles, V, usable)
    ref = np.zeros(V, dtype=bool)
    ref[t[valid].reshape(-1)] = True
    members = np.flatnonzero(ref)
    key = ((i[:, 0] + LIMIT) | ((i[:, 1] + LIMIT) << 21) | ((i[:, 2] + LIMIT) << 42)).astype(np.uint64)
    # clusters: the referenced vertices of one cell; leader = the smallest index (members is ascending: first occurrence)
    uniq, first, inverse = np.unique(key[members], return_index=True, return_inverse=True)
    lead = np.full(V, -1, dtype=np.int64)
    lead[members] = members[first][inverse]
    n_clusters = len(uniq)
    # the mean, from exact integer sums
    two32 = np.float64(4294967296.0)
    q = np.floor(f * two32).astype(np.uint64)
    S = np.zeros((V, 3), dtype=np.uint64)
    n = np.zeros(V, dtype=np.uint64)
    np.add.at(S, lead[members], q[members])
    np.add.at(n, lead[members], np.uint64(1))
    with np.errstate(all="ignore"):
        a = S.astype(np.float64) / n.astype(np.float64)[:, None]
        m = a * np.float64(2.0 ** -32)
        ml = m[np.maximum(lead, 0)]
        dx = f[:, 0] - ml[:, 0]
        dy = f[:, 1] - ml[:, 1]
        dz = f[:, 2] - ml[:, 2]
        xx = dx * dx
        yy = dy * dy
        zz = dz * dz
        xy = xx + yy
        d2 = xy + zz
    bits = d2.view(np.uint64)
    # representative: min of (d2 bits, index) among the members
    best = np.full(V, np.iinfo(np.uint64).max, dtype=np.uint64)
    np.minimum.at(best, lead[members], bits[members])
    rep = np.full(V, V, dtype=np.int64)
    winners = members[bits[members] == best[lead[members]]]
    np.minimum.at(rep, lead[winners], winners)
    # triangles
    lt = lead[np.where(valid[:, None], t, 0)] if V else np.zeros((len(t), 3), dtype=np.int64)
    degenerate = valid & ((lt[:, 0] == lt[:, 1]) | (lt[:, 1] == lt[:, 2]) | (lt[:, 0] == lt[:, 2]))
    enters = valid & ~degenerate
    idx = np.flatnonzero(enters)
    survive = np.zeros(len(t), dtype=bool)
    if len(idx):
        _, first_t = np.unique(np.sort(lt[idx], axis=1), axis=0, return_index=True)      # first occurrence = smallest index
        survive[idx[first_t]] = True
    # a surviving triangle is remapped through the cluster of each corner
    tl = t.copy()
    return _assemble(v, tl, V, lead, rep, survive,
                     [int(degenerate.sum()), int(enters.sum() - survive.sum()), flags, n_clusters], origin)


def simplify_brute(vertices, triangles, cell_size, origin=None):
    """The same result the slow way: a Python loop over the distinct cell triples, Python sets for the duplicates, the
    mean from Python integers."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    V = len(v)
    origin = default_origin(v) if origin is None else np.asarray(origin, dtype=np.float64)
    i, f, usable = cells(v, origin, cell_size)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    flags = 0
    valid = []
    for a, b, c in t.tolist():
        if min(a, b, c) < 0 or max(a, b, c) >= V:
            flags |= FLAG_BAD_INDEX
            valid.append(False)
        elif not (usable[a] and usable[b] and usable[c]):
            flags |= FLAG_BAD_VERTEX
            valid.append(False)
        else:
            valid.append(True)
    valid = np.array(valid, dtype=bool)
    referenced = sorted(set(t[valid].reshape(-1).tolist()))
    lead = np.full(V, -1, dtype=np.int64)
    rep = np.full(V, V, dtype=np.int64)
    n_clusters = 0
    if referenced:
        r = np.array(referenced)
        for cell in np.unique(i[r], axis=0):
            mem = r[(i[r] == cell).all(axis=1)]
            n_clusters += 1
            lead[mem] = mem.min()
            q = [[int(np.floor(f[j, d] * 4294967296.0)) for d in range(3)] for j in mem]
            mean = [np.float64(sum(row[d] for row in q)) / np.float64(len(mem)) * np.float64(2.0 ** -32) for d in range(3)]
            dev = [[f[j, d] - mean[d] for d in range(3)] for j in mem]
            d2 = [(e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] for e in dev]
            rep[mem.min()] = min(zip(d2, mem.tolist()))[1]
    survive = np.zeros(len(t), dtype=bool)
    seen = set()
    n_degenerate = n_duplicate = 0
    for k, (a, b, c) in enumerate(t.tolist()):
        if not valid[k]:
            continue
        triple = (lead[a], lead[b], lead[c])
        if len(set(triple)) < 3:
            n_degenerate += 1
        elif frozenset(triple) in seen:
            n_duplicate += 1
        else:
            seen.add(frozenset(triple))
            survive[k] = True
    return _assemble(v, t, V, lead, rep, survive, [n_degenerate, n_duplicate, flags, n_clusters], origin)


def equal(a, b):
    """two results agree exactly (coordinates as bits, NaN included)"""
    return (all(np.array_equal(a[k], b[k]) and a[k].shape == b[k].shape and a[k].dtype == b[k].dtype
                for k in ("triangles", "vertex_index", "vertex_cluster", "triangle_index"))
            and np.array_equal(a["vertices"], b["vertices"], equal_nan=True) and a["counts"] == b["counts"])


def target_grid(vertices):
    """(origin, L) of `target_triangles`: the box of the finite vertices"""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    ok = np.isfinite(v).all(axis=1)
    lo, hi = v[ok].min(axis=0), v[ok].max(axis=0)
    return lo, float((hi - lo).max())


def hub(double):
    """4,096 fan triangles round vertex 0, every other vertex in a cell of its own at cell size 1"""
    k = 4096
    j = np.arange(2 * k)
    others = np.stack([2.0 + (j % 128) + 0.25, 2.0 + (j // 128) + 0.5, np.full(2 * k, 3.75)], axis=1)
    v = np.concatenate([[[0.5, 0.5, 0.5]], others])
    t = np.stack([np.zeros(k, dtype=np.int64), 1 + 2 * np.arange(k), 2 + 2 * np.arange(k)], axis=1).astype(np.int32)
    if double:                                                # every triangle twice, the copy turned round
        t = np.stack([t, t[:, ::-1]], axis=1).reshape(-1, 3)
    return v, t
