"""Brute-force fp64 numpy reference of the mesh ray casting (csrc/mesh_raycast.hip): the first hit of every ray over ALL
triangles under the order (t as computed, triangle index), and the shapes and rays the tests share.  Not a test module.

THE PAIR TEST is `ray_triangle`: the watertight test of Woop, Benthin and Wald (JCGT 2013) in fp64 as include/rnbneus.h
spells it out, operation for operation — numpy rounds every product and difference on its own, and the kernel is
compiled without contraction, so device and reference are required to agree BIT FOR BIT, triangle indices included.
`ray_triangle_mt` is a second, independent formulation (Moeller and Trumbore) for cross-checking rays well inside a
triangle; on edges and vertices of a closed surface it leaves pinholes, which is why it is not the kernel's test."""
import numpy as np

from tests.mesh_distance_ref import usable

EPS = 2.0 ** -52


def ray_setup(o, d):
    """(kx, ky, kz [N] int, Sx, Sy, Sz [N]) of rays o + t d ([N,3])"""
    d = np.asarray(d, dtype=np.float64)
    kz = np.argmax(np.abs(d), axis=1)                      # the first maximum
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    rows = np.arange(len(d))
    swap = d[rows, kz] < 0.0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dz = d[rows, kz]
        return kx, ky, kz, d[rows, kx] / dz, d[rows, ky] / dz, 1.0 / dz


def ray_triangle(o, d, a, b, c, t_min, t_max):
    """rays o, d [N,3], bounds [N] against triangles a, b, c [T,3]: (hit [N,T] bool, t, U, V, W, det [N,T])"""
    o = np.asarray(o, dtype=np.float64)
    kx, ky, kz, Sx, Sy, Sz = ray_setup(o, d)
    rows = np.arange(len(o))
    ox, oy, oz = o[rows, kx][:, None], o[rows, ky][:, None], o[rows, kz][:, None]
    Sx, Sy, Sz = Sx[:, None], Sy[:, None], Sz[:, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        sheared = []
        for p in (a, b, c):
            p = np.asarray(p, dtype=np.float64)
            pkz = p[:, kz].T - oz                           # [N,T]: the corner's kz coordinate of every ray, translated
            sheared.append(((p[:, kx].T - ox) - Sx * pkz, (p[:, ky].T - oy) - Sy * pkz, Sz * pkz))
        (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = sheared
        U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        inside = ((U >= 0.0) & (V >= 0.0) & (W >= 0.0)) | ((U <= 0.0) & (V <= 0.0) & (W <= 0.0))
        det = (U + V) + W
        t = ((U * Az + V * Bz) + W * Cz) / det
        hit = inside & (det != 0.0) & (t >= np.asarray(t_min)[:, None]) & (t <= np.asarray(t_max)[:, None])
    return hit, t, U, V, W, det


def ray_triangle_mt(o, d, a, b, c, t_min, t_max):
    """Moeller-Trumbore: (hit [N,T], t [N,T]); an edge or vertex hit may be lost on both sides"""
    o, d = np.asarray(o, dtype=np.float64)[:, None, :], np.asarray(d, dtype=np.float64)[:, None, :]
    e1, e2 = (b - a)[None], (c - a)[None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pv = np.cross(d, e2)
        det = (e1 * pv).sum(-1)
        tv = o - a[None]
        u = (tv * pv).sum(-1) / det
        qv = np.cross(tv, e1)
        v = (d * qv).sum(-1) / det
        t = (e2 * qv).sum(-1) / det
        hit = (det != 0.0) & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0) & (t >= np.asarray(t_min)[:, None]) & (t <= np.asarray(t_max)[:, None])
    return hit, t


def _bounds(N, t_min, t_max):
    lo = np.zeros(N) if t_min is None else np.broadcast_to(np.asarray(t_min, dtype=np.float64), (N,)).copy()
    hi = np.full(N, np.inf) if t_max is None else np.broadcast_to(np.asarray(t_max, dtype=np.float64), (N,)).copy()
    return lo, hi


def valid_rays(o, d, lo, hi):
    return np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0.0).any(axis=1) & ~np.isnan(lo) & ~np.isnan(hi)


def raycast_all(origins, directions, vertices, triangles, t_min=None, t_max=None, fn="watertight", chunk=512):
    """(t [N], triangle [N] int32, bary [N,3]) over all usable triangles under the order (t, index).  No hit: (+inf, -1,
    NaN); a ray with a non-finite origin or direction, a zero direction or a NaN bound: (NaN, -1, NaN).
    fn = "mt": Moeller-Trumbore (bary is NaN)."""
    o = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    v, tri = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    N = len(o)
    lo, hi = _bounds(N, t_min, t_max)
    ok = valid_rays(o, d, lo, hi)
    ids = np.flatnonzero(usable(v, tri))
    t_out, tr_out, bary = np.full(N, np.inf), np.full(N, -1, dtype=np.int32), np.full((N, 3), np.nan)
    safe_o, safe_d = np.where(ok[:, None], o, 0.0), np.where(ok[:, None], d, 1.0)
    if len(ids):
        a, b, c = (v[tri[ids, k]] for k in range(3))
        for s in range(0, N, chunk):
            e = slice(s, s + chunk)
            if fn == "mt":
                hit, t = ray_triangle_mt(safe_o[e], safe_d[e], a, b, c, lo[e], hi[e])
                U = V = W = det = np.full(t.shape, np.nan)
            else:
                hit, t, U, V, W, det = ray_triangle(safe_o[e], safe_d[e], a, b, c, lo[e], hi[e])
            tt = np.where(hit, t, np.inf)
            j = np.argmin(tt, axis=1)                       # the first minimum: the smallest triangle index
            rows = np.arange(len(j))
            found = tt[rows, j] < np.inf
            t_out[e] = np.where(found, t[rows, j], np.inf)
            tr_out[e] = np.where(found, ids[j], -1)
            with np.errstate(invalid="ignore", divide="ignore"):
                bb = np.stack([U[rows, j], V[rows, j], W[rows, j]], axis=1) / det[rows, j][:, None]
            bary[e] = np.where(found[:, None], bb, np.nan)
    t_out[~ok], tr_out[~ok], bary[~ok] = np.nan, -1, np.nan
    return t_out, tr_out, bary


def face_normals(vertices, triangles):
    v, t = np.asarray(vertices, dtype=np.float64), np.asarray(triangles, dtype=np.int64)
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    with np.errstate(invalid="ignore", divide="ignore"):
        return n / np.sqrt((n * n).sum(axis=1))[:, None]


# ---- shapes and rays, computed once and shared (callers must not modify them) -----------------------------------------

_CASES = {}


def icosphere(subdivisions=2):
    """(vertices [V,3] float64 on the unit sphere, triangles [T,3] int32, outward): 12 / 20, 42 / 80, 162 / 320, ..."""
    key = ("ico", subdivisions)
    if key not in _CASES:
        p = (1.0 + 5.0 ** 0.5) / 2.0
        v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
             (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
        v = [np.array(x, dtype=np.float64) / np.sqrt(1.0 + p * p) for x in v]
        f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
             (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
             (9, 8, 1)]
        for _ in range(subdivisions):
            mid, nf = {}, []

            def midpoint(i, j):
                k = (min(i, j), max(i, j))
                if k not in mid:
                    m = v[i] + v[j]
                    v.append(m / np.sqrt(m @ m))
                    mid[k] = len(v) - 1
                return mid[k]

            for a, b, c in f:
                ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
                nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
            f = nf
        _CASES[key] = (np.ascontiguousarray(v), np.ascontiguousarray(f, dtype=np.int32))
    return _CASES[key]


def mesh_edges(triangles):
    t = np.asarray(triangles, dtype=np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0)


ICO_ORIGINS = np.array([[0.0, 0.0, 0.0], [0.31, -0.17, 0.23], [-0.05, 0.44, -0.12]])


def watertight_case():
    """The closed-surface case: the twice-subdivided icosphere (162 vertices, 320 triangles, 480 edges) and, from each of
    three interior origins, the rays through every vertex, every edge midpoint and four random points per edge:
    2,562 rays per origin, `origins`, `directions` [3 x 2562, 3] with t = 1 at the target, and the reference's `ref`."""
    if "watertight" not in _CASES:
        v, t = icosphere(2)
        e = mesh_edges(t)
        assert v.shape == (162, 3) and t.shape == (320, 3) and e.shape == (480, 2)
        rng = np.random.default_rng(7)
        s = rng.uniform(0.0, 1.0, (480, 4, 1))
        on_edges = (v[e[:, 0]][:, None] + s * (v[e[:, 1]] - v[e[:, 0]])[:, None]).reshape(-1, 3)
        targets = np.concatenate([v, 0.5 * (v[e[:, 0]] + v[e[:, 1]]), on_edges])
        assert len(targets) == 2562
        o = np.repeat(ICO_ORIGINS, len(targets), axis=0)
        d = np.tile(targets, (3, 1)) - o
        _CASES["watertight"] = {"vertices": v, "triangles": t, "origins": np.ascontiguousarray(o),
                                "directions": np.ascontiguousarray(d), "ref": raycast_all(o, d, v, t)}
    return _CASES["watertight"]


def torus_rays():
    """The parity case on the torus of mesh_distance_ref.torus_mesh() (1,200 triangles), about 2,000 rays: 500 from inside
    the tube outwards, 500 from outside towards points of the surface, 300 that pass the mesh's box by, 300 segments
    whose t_max ends short of the surface (and 100 that end exactly on it), 300 that start ON the surface (a centroid,
    t_min = 0) and leave along a random direction.  A dict with `origins`, `directions`, `t_min`, `t_max` and `ref`."""
    if "torus" not in _CASES:
        from tests.mesh_distance_ref import torus_mesh
        v, t = torus_mesh()
        rng = np.random.default_rng(21)
        cen = v[t].mean(axis=1)

        def unit(n):
            x = rng.normal(size=(n, 3))
            return x / np.sqrt((x * x).sum(axis=1))[:, None]

        phi = rng.uniform(0.0, 2.0 * np.pi, 500)
        core = np.stack([0.55 * np.cos(phi), 0.55 * np.sin(phi), np.zeros(500)], axis=1) + 0.05 * rng.uniform(-1, 1, (500, 3))
        o1, d1 = core, unit(500) * rng.uniform(0.5, 2.0, (500, 1))
        o2 = unit(500) * rng.uniform(1.5, 4.0, (500, 1))
        d2 = cen[rng.integers(0, len(cen), 500)] + 0.01 * rng.normal(size=(500, 3)) - o2
        o3 = unit(300) * 3.0
        d3 = np.cross(o3, unit(300))                        # tangent to the sphere of radius 3: never near the box
        o4 = unit(400) * rng.uniform(1.5, 3.0, (400, 1))
        tgt = cen[rng.integers(0, len(cen), 400)]
        d4 = tgt - o4                                       # t = 1 at a centroid (on the surface up to rounding)
        o5 = cen[rng.integers(0, len(cen), 300)]
        d5 = unit(300)
        o = np.concatenate([o1, o2, o3, o4, o5])
        d = np.concatenate([d1, d2, d3, d4, d5])
        lo, hi = np.zeros(len(o)), np.full(len(o), np.inf)
        full = raycast_all(o4, d4, v, t)[0]                 # where the segments would first hit
        hi[1300:1600] = full[:300] * rng.uniform(0.2, 0.999, 300)
        hi[1600:1700] = full[300:]                          # t_max == t: inclusive
        lo[1000:1300:2] = -np.inf                           # lines, for half of the passers-by
        _CASES["torus"] = {"vertices": v, "triangles": t, "origins": np.ascontiguousarray(o), "directions": np.ascontiguousarray(d),
                           "t_min": lo, "t_max": hi, "ref": raycast_all(o, d, v, t, lo, hi)}
    return _CASES["torus"]


def pinhole_rays(H, W, eye, look_at, fov_deg=40.0):
    """(origins, directions) [H*W,3] of a pinhole view, row-major, directions NOT normalised (z = 1 in the camera frame)"""
    eye, look_at = np.asarray(eye, dtype=np.float64), np.asarray(look_at, dtype=np.float64)
    fwd = (look_at - eye) / np.linalg.norm(look_at - eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    f = 0.5 * W / np.tan(np.radians(0.5 * fov_deg))
    ys, xs = np.meshgrid(np.arange(H) + 0.5 - 0.5 * H, np.arange(W) + 0.5 - 0.5 * W, indexing="ij")
    d = fwd[None] + (xs.reshape(-1, 1) / f) * right[None] - (ys.reshape(-1, 1) / f) * up[None]
    return np.ascontiguousarray(np.tile(eye, (H * W, 1))), np.ascontiguousarray(d)
