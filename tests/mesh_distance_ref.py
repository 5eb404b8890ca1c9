"""Brute-force fp64 numpy reference of the mesh evaluation (csrc/mesh_eval.hip): squared distance, closest point and
triangle of every query over ALL triangles, and the pieces the sampling tests rebuild on the host.  Not a test module.

THE SQUARED DISTANCE point-triangle is `point_triangle`: the minimum of |p - q|^2 over q = the closest point of each of
the three clamped edge segments and, where the triangle has a normal and the projection of p onto its plane has
barycentric weights >= 0, that projection.  It is defined for zero-area triangles (the segment or point they degenerate
to), and the kernel evaluates the same expression operation for operation.  `point_triangle_ericson` is a second,
independent formulation (the Voronoi-region test of Ericson, Real-Time Collision Detection, 5.1.5) for cross-checking
on non-degenerate triangles.

THE TOLERANCE RULE, used everywhere: compare SQUARED distances,
    |d2 - d2_ref| <= 16 * 2^-52 * L^2,    L = max |query coordinate| + max |vertex coordinate|.
Why squared: d2 = |p - q|^2 with q rounded to ~2^-53 L per coordinate carries an error of ~d 2^-52 L, so near the surface
(d -> 0) a bound on d itself would have to be of the order of sqrt(2^-52) L.  Every intermediate (edge vectors, the
parameter, q) is good to a few 2^-53 L, and d <= 2 L, which puts two evaluation orders of the same pair a few 2^-52 L^2
apart; 16 leaves room for a third.  Triangle indices are never compared for equality — most queries near a mesh tie
between neighbouring triangles at an edge or a vertex, and the tie may break differently for two evaluation orders;
instead the returned closest point must lie on the returned triangle and be dist2 away (`check_closest`)."""
import numpy as np

EPS = 2.0 ** -52
U64 = (1 << 64) - 1


def bound(queries, vertices):
    """16 * 2^-52 * L^2 over the finite coordinates"""
    q, v = np.asarray(queries, dtype=np.float64), np.asarray(vertices, dtype=np.float64)
    m = lambda x: float(np.abs(x[np.isfinite(x)]).max()) if np.isfinite(x).any() else 0.0   # noqa: E731
    L = m(q) + m(v)
    return 16.0 * EPS * L * L


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _segment(p, a, b):
    ab, ap = b - a, p - a
    dd = _dot(ab, ab)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(dd > 0.0, _dot(ap, ab) / dd, 0.0)
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    q = a + t[..., None] * ab
    r = p - q
    return _dot(r, r), q


def point_triangle(p, a, b, c):
    """(d2, q) for broadcastable [...,3] arrays: the definition in the module docstring, candidates in the order interior,
    ab, bc, ca, the first strict minimum wins"""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (p, a, b, c)))
    ab, ac, ap = b - a, c - a, p - a
    n = _cross(ab, ac)
    nn = _dot(n, n)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        wb = _dot(_cross(ap, ac), n) / nn
        wc = _dot(_cross(ab, ap), n) / nn
    wa = (1.0 - wb) - wc
    inside = (nn > 0.0) & (wa >= 0.0) & (wb >= 0.0) & (wc >= 0.0)
    with np.errstate(invalid="ignore"):
        q = (a + wb[..., None] * ab) + wc[..., None] * ac
        r = p - q
        best = np.where(inside, _dot(r, r), np.inf)
    bq = np.where(inside[..., None], q, np.nan)
    for u, v in ((a, b), (b, c), (c, a)):
        d2, q = _segment(p, u, v)
        take = d2 < best
        best = np.where(take, d2, best)
        bq = np.where(take[..., None], q, bq)
    return best, bq


def point_triangle_ericson(p, a, b, c):
    """(d2, q): Ericson's region test, for triangles with a normal"""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (p, a, b, c)))
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - b
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p - c
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / (va + vb + vc)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    with np.errstate(invalid="ignore"):
        cands = [a, b, a + v_ab[..., None] * ab, c, a + w_ac[..., None] * ac, b + w_bc[..., None] * (c - b),
                 a + ab * (vb * den)[..., None] + ac * (vc * den)[..., None]]
    q = cands[-1]
    for cond, cand in zip(reversed(conds), reversed(cands[:-1])):
        q = np.where(cond[..., None], cand, q)
    r = p - q
    return _dot(r, r), q


def usable(vertices, triangles):
    """[T] bool: every index inside [0, V) and every coordinate finite (the others are skipped by the library)"""
    v, t = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    ok = ((t >= 0) & (t < len(v))).all(axis=1)
    fin = np.isfinite(v).all(axis=1)
    ok[ok] = fin[t[ok]].all(axis=1)
    return ok


def closest_all(queries, vertices, triangles, fn=point_triangle, chunk=256):
    """(dist2 [N], closest [N,3], triangle [N] int32) over all usable triangles under the order (dist2, index); a query
    with a non-finite coordinate gets (NaN, NaN, -1), a mesh without usable triangles (+inf, NaN, -1)"""
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    v, t = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    ids = np.flatnonzero(usable(v, t))
    N = len(q)
    d2, cl, tr = np.full(N, np.inf), np.full((N, 3), np.nan), np.full(N, -1, dtype=np.int32)
    if len(ids):
        a, b, c = (v[t[ids, k]][None] for k in range(3))
        for s in range(0, N, chunk):
            p = np.nan_to_num(q[s:s + chunk, None, :], nan=0.0, posinf=0.0, neginf=0.0)
            dd, qq = fn(p, a, b, c)
            j = np.argmin(dd, axis=1)                       # the first minimum: the smallest triangle index
            rows = np.arange(len(j))
            d2[s:s + chunk], cl[s:s + chunk], tr[s:s + chunk] = dd[rows, j], qq[rows, j], ids[j]
    bad = ~np.isfinite(q).all(axis=1)
    d2[bad], cl[bad], tr[bad] = np.nan, np.nan, -1
    return d2, cl, tr


def check_closest(name, queries, vertices, triangles, got, ref_d2, tol):
    """The parity rule: got = (dist2, closest, triangle) arrays of a device query.  dist2 within tol of the reference; the
    returned closest point lies on the returned triangle (its reference squared distance to it <= tol) and is dist2 away
    from the query (|p - closest|^2 within tol of dist2).  Returns the worst error as a fraction of tol."""
    q, v, t = np.asarray(queries, dtype=np.float64), np.asarray(vertices, dtype=np.float64), np.asarray(triangles, dtype=np.int64)
    d2, cl, tr = (np.asarray(x) for x in got)
    assert d2.shape == ref_d2.shape and cl.shape == q.shape and tr.shape == ref_d2.shape, name
    fin = np.isfinite(ref_d2)
    assert np.array_equal(np.isnan(d2), np.isnan(ref_d2)) and np.array_equal(np.isposinf(d2), np.isposinf(ref_d2)), name
    assert (tr[~fin] == -1).all() and np.isnan(cl[~fin]).all(), name
    ok = usable(v, t)
    assert (tr[fin] >= 0).all() and (tr[fin] < len(t)).all() and ok[tr[fin]].all(), f"{name}: triangle index"
    e_ref = np.abs(d2[fin] - ref_d2[fin])
    corners = v[t[tr[fin]]]
    on_tri = point_triangle(cl[fin], corners[:, 0], corners[:, 1], corners[:, 2])[0]
    r = q[fin] - cl[fin]
    e_len = np.abs(_dot(r, r) - d2[fin])
    worst = max(float(x.max()) if x.size else 0.0 for x in (e_ref, on_tri, e_len)) / tol
    print(f"{name}: {int(fin.sum())} queries, |dist2 - ref| {e_ref.max() if e_ref.size else 0:.3e}, closest off its triangle "
          f"{on_tri.max() if on_tri.size else 0:.3e}, | |p - closest|^2 - dist2 | {e_len.max() if e_len.size else 0:.3e}; "
          f"worst = {worst:.3f} of 16 x 2^-52 L^2 = {tol:.3e}")
    assert (e_ref <= tol).all(), f"{name}: dist2 is {e_ref.max() / tol:.2f} of the bound from the reference"
    assert (on_tri <= tol).all(), f"{name}: a closest point is off its triangle by {on_tri.max() / tol:.2f} of the bound"
    assert (e_len <= tol).all(), f"{name}: |p - closest|^2 differs from dist2 by {e_len.max() / tol:.2f} of the bound"
    return worst


def torus_distance(p, R=0.55, r=0.22):
    """unsigned distance to the torus of tests/mc_shapes.torus (axis z)"""
    p = np.asarray(p, dtype=np.float64)
    return np.abs(np.sqrt((np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - R) ** 2 + p[..., 2] ** 2) - r)


def to_model(verts, n, lo=-1.0, hi=1.0):
    """grid-index vertices of a marching-cubes mesh over an n^3 grid -> the coordinates of tests/mc_shapes._grid"""
    return np.ascontiguousarray(np.asarray(verts, dtype=np.float64) / (n - 1) * (hi - lo) + lo)


_CASES = {}
TORUS_N = 20


def torus_mesh():
    """(vertices [V,3] float64 in model coordinates, triangles [1200,3] int32) of mc_shapes.torus(20), once"""
    if "mesh" not in _CASES:
        from oracle import mc_oracle
        from tests import mc_shapes
        v, t = mc_oracle.marching_cubes(mc_shapes.torus(TORUS_N), 0.0)
        _CASES["mesh"] = (to_model(v, TORUS_N), np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3))
    return _CASES["mesh"]


def torus_case():
    """The parity case, computed once and shared (callers must not modify it): a dict with the torus mesh `vertices`,
    `triangles`; `queries` = 1,500 uniform points of [-1.3, 1.3]^3 (many outside the mesh's box), every vertex, every
    centroid, every centroid moved 1e-9 along its face normal; `far` = one query 50 box sizes away (checked under its own
    L); and the brute-force reference of both (`ref`, `ref_far`: dist2, closest, triangle)."""
    if "case" not in _CASES:
        v, t = torus_mesh()
        rng = np.random.default_rng(20)
        a, b, c = (v[t[:, k]] for k in range(3))
        cen = (a + b + c) / 3.0
        n = _cross(b - a, c - a)
        n /= np.sqrt(_dot(n, n))[:, None]
        q = np.ascontiguousarray(np.concatenate([rng.uniform(-1.3, 1.3, (1500, 3)), v, cen, cen + 1e-9 * n]))
        far = np.array([[50.0 * 1.6, -31.0, 12.5]])
        _CASES["case"] = {"vertices": v, "triangles": t, "queries": q, "far": far, "ref": closest_all(q, v, t),
                          "ref_far": closest_all(far, v, t)}
    return _CASES["case"]


# ---- surface samples: the pieces a caller needs to reproduce a sample (include/rnbneus.h) -----------------------------

def triangle_areas(vertices, triangles):
    """A_t = 0.5 |(b - a) x (c - a)|, 0 for an unusable triangle"""
    v, t = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    ok = usable(v, t)
    out = np.zeros(len(t))
    a, b, c = (v[t[ok, k]] for k in range(3))
    n = _cross(b - a, c - a)
    out[ok] = 0.5 * np.sqrt(_dot(n, n))
    return out


def mix(z):
    """the integer mixer on Python ints (unsigned 64-bit)"""
    z = (z + 0x9E3779B97F4A7C15) & U64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & U64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & U64
    return z ^ (z >> 31)


def unit(z):
    return float(z >> 11) * 2.0 ** -53


def sample_bary(seed, k):
    """the barycentric weights of sample k"""
    s = mix(seed & U64)
    r1, r2 = unit(mix(s ^ (2 * k))), unit(mix(s ^ (2 * k + 1)))
    if 1.0 - r1 < r2:
        r1, r2 = 1.0 - r1, 1.0 - r2
    return ((1.0 - r1) - r2, r1, r2)


def sample_offset(seed):
    """xi of the systematic sample positions u_k = ((k + xi) A) / n"""
    return unit(mix(seed & U64))


def spread_mesh():
    """2,500 separate triangles (three scan tiles) whose areas span 10^6, with zero-area triangles at the places a scan can
    get wrong: first, either side of a tile boundary, last"""
    rng = np.random.default_rng(11)
    T = 2500
    size = np.sqrt(np.logspace(-3.0, 3.0, T))
    rng.shuffle(size)
    a = rng.uniform(-50.0, 50.0, (T, 3))
    e1, e2 = rng.standard_normal((T, 3)), rng.standard_normal((T, 3))
    b, c = a + size[:, None] * e1, a + size[:, None] * e2
    zero = np.array([0, 1023, 1024, 1700, T - 1])
    c[zero] = b[zero]                                             # two equal corners: the cross product is exactly 0
    c[1700] = b[1700] = a[1700]                                   # a point
    v = np.stack([a, b, c], axis=1).reshape(-1, 3)
    return v, np.arange(3 * T, dtype=np.int32).reshape(-1, 3), zero
