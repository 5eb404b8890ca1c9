"""The texture atlas of rnb_texture_* (include/rnbneus.h "Texture baking") restated in numpy, operation for operation: the
layout, the owner and lattice coordinate of a texel, the sample numbering r(a1, a2) and its inverse, the sample points, the
pack's two image rules, and the bilinear lookup with the texels it reads.  numpy only; not a test module.

Everything integer is int64; the sample points are float64 with every product, quotient and sum rounded on its own (numpy
never contracts), converted to float32 at the end; the normal quantisation is float32 throughout."""
import numpy as np


def n_samples(s):
    return (s + 1) * (s + 2) // 2


def layout(T, size=None, chart=None):
    """dict(s, c, cols, rows, W, H, samples_per_triangle) of `atlas_layout`; ValueError where it raises"""
    K = (T + 1) // 2
    if size is None:
        s = 8 if chart is None else int(chart)
        if not 1 <= s <= 255:
            raise ValueError("chart")
        c = s + 5
        cols = 0
        while cols * cols < K:       # ceil(sqrt(K)) in integers
            cols += 1
        rows = (K + cols - 1) // cols if cols else 0
        return dict(s=s, c=c, cols=cols, rows=rows, W=cols * c, H=rows * c, samples_per_triangle=n_samples(s))
    size = int(size)
    cands = range(255, 0, -1) if chart is None else [int(chart)]
    for s in cands:
        if not 1 <= s <= 255:
            raise ValueError("chart")
        c = s + 5
        cols = size // c
        if cols * (size // c) >= K and size >= 1:
            rows = (K + cols - 1) // cols if cols else 0
            return dict(s=s, c=c, cols=cols, rows=rows, W=size, H=size, samples_per_triangle=n_samples(s))
    raise ValueError("size")


def corner_texels(L, T):
    """[T,3,2] int64: the texel (x, y) of every triangle corner in the image"""
    s, c, cols = L["s"], L["c"], max(L["cols"], 1)
    t = np.arange(T, dtype=np.int64)
    k = t // 2
    x0, y0 = (k % cols) * c, (k // cols) * c
    up = (t % 2 == 1)
    lo = np.array([[1, 1], [1 + s, 1], [1, 1 + s]], dtype=np.int64)
    hi = np.array([[c - 2, c - 2], [c - 2 - s, c - 2], [c - 2, c - 2 - s]], dtype=np.int64)
    local = np.where(up[:, None, None], hi[None], lo[None])
    return local + np.stack([x0, y0], axis=1)[:, None, :]


def uv(L, T):
    """[T,3,2] float64: u = (x + 0.5) / W, v = 1 - (y + 0.5) / H of the corner texels"""
    xy = corner_texels(L, T).astype(np.float64)
    if T == 0:
        return np.zeros((0, 3, 2))
    return np.stack([(xy[..., 0] + 0.5) / np.float64(L["W"]), 1.0 - (xy[..., 1] + 0.5) / np.float64(L["H"])], axis=-1)


def cell_owner(s, i, j):
    """inside a cell: (upper half? (bool), a1, a2) of the texel indices i, j in [0, s + 5)"""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    c = s + 5
    up = (i + j) > s + 3
    a1 = np.clip(np.where(up, c - 2 - i, i - 1), 0, s)
    a2 = np.where(up, c - 2 - j, j - 1)
    a2 = np.minimum(np.maximum(a2, 0), s - a1)
    return up, a1, a2


def rank(s, a1, a2):
    """r(a1, a2): rows of constant a2"""
    a1, a2 = np.asarray(a1, dtype=np.int64), np.asarray(a2, dtype=np.int64)
    return a2 * (s + 1) - a2 * (a2 - 1) // 2 + a1


def unrank(s, r):
    """(a1, a2) of r in [0, n_s): a2 = the last row whose first rank is <= r"""
    r = np.asarray(r, dtype=np.int64)
    a2 = np.zeros_like(r)
    for row in range(s + 1):
        a2 = np.where(rank(s, 0, row) <= r, row, a2)
    return r - rank(s, 0, a2), a2


def bad_triangles(vertices, triangles):
    """[T] bool: an index outside [0, V) or a non-finite corner"""
    v, t = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    V = len(v)
    bad = ((t < 0) | (t >= V)).any(axis=1)
    if V:
        fin = np.isfinite(v).all(axis=1)
        bad |= ~fin[np.clip(t, 0, V - 1)].all(axis=1)
    return bad


def sample_points(vertices, triangles, s, first=0, count=None):
    """(points [count,3] float32, number of bad triangles whose sample r = 0 lies in the range)"""
    v, t = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    ns = n_samples(s)
    count = len(t) * ns - first if count is None else count
    p = first + np.arange(count, dtype=np.int64)
    tri, r = p // ns, p % ns
    a1, a2 = unrank(s, r)
    bad = bad_triangles(v, t)
    sd = np.float64(s)
    w1, w2, w0 = a1.astype(np.float64) / sd, a2.astype(np.float64) / sd, (s - a1 - a2).astype(np.float64) / sd
    idx = np.clip(t[tri], 0, max(len(v) - 1, 0))
    if len(v) == 0:
        return np.zeros((count, 3), dtype=np.float32), int((bad[tri] & (r == 0)).sum())
    A, B, C = v[idx[:, 0]], v[idx[:, 1]], v[idx[:, 2]]
    with np.errstate(invalid="ignore", over="ignore"):
        P = (w0[:, None] * A + w1[:, None] * B) + w2[:, None] * C
        P = np.where(bad[tri][:, None], 0.0, P).astype(np.float32)
    return P, int((bad[tri] & (r == 0)).sum())


def texel_map(L, T, bad=None):
    """(texel_sample [H,W] int32: -1 where empty or the triangle is bad; owner [H,W] int64: the triangle of the texel's
    half-cell whether it exists or not, -1 right of the cells)"""
    s, c, cols, W, H = L["s"], L["c"], L["cols"], L["W"], L["H"]
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    cx, cy = x // c, y // c
    up, a1, a2 = cell_owner(s, x - cx * c, y - cy * c)
    t = 2 * (cy * cols + cx) + up
    inside = cx < cols
    owner = np.where(inside, t, -1)
    live = inside & (t < T)
    if bad is not None and T:
        live &= ~np.asarray(bad)[np.clip(t, 0, T - 1)]
    sample = np.where(live, t * n_samples(s) + rank(s, a1, a2), -1)
    return sample.astype(np.int32), owner


def quantize_normal(n):
    """uint8 of float32 normals: rint(255 (0.5 n + 0.5)) clipped to [0, 255], every operation in float32; NaN gives 0"""
    n = np.asarray(n, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (np.float32(0.5) * n + np.float32(0.5)) * np.float32(255.0)
        q = np.where(v >= 0, np.where(v <= 255, np.rint(v), np.float32(255.0)), np.float32(0.0))
    return q.astype(np.uint8)


def pack(L, vertices, triangles, rgb=None, normal=None):
    """(albedo_image [H,W,4] uint8 or None, normal_image [H,W,4] uint8 or None, texel_sample [H,W] int32)"""
    T = len(np.asarray(triangles).reshape(-1, 3))
    sample, _ = texel_map(L, T, bad_triangles(vertices, triangles))
    live = sample >= 0
    idx = np.clip(sample, 0, None)
    out = []
    for src in (None if rgb is None else np.asarray(rgb, dtype=np.uint8), None if normal is None else quantize_normal(normal)):
        if src is None:
            out.append(None)
            continue
        img = np.zeros((L["H"], L["W"], 4), dtype=np.uint8)
        if live.any():
            img[..., :3] = np.where(live[..., None], src[idx], 0)
            img[..., 3] = np.where(live, 255, 0)
        out.append(img)
    return out[0], out[1], sample


def bilinear_taps(px, py):
    """the four taps of a bilinear lookup at texel-centre coordinates (px, py) (texel x has its centre at px = x):
    (x [n,4], y [n,4], weight [n,4])"""
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    x0, y0 = np.floor(px), np.floor(py)
    fx, fy = px - x0, py - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xs = np.stack([x0, x0 + 1, x0, x0 + 1], axis=-1)
    ys = np.stack([y0, y0, y0 + 1, y0 + 1], axis=-1)
    ws = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], axis=-1)
    return xs, ys, ws


def lookup(image, uv_corners, triangle, bary):
    """`sample_texture` in numpy: image [H,W,C] (any dtype, read as float64), uv_corners [T,3,2], triangle [N], bary [N,3]:
    [N,C] float64, NaN rows for triangle < 0.  Taps are clamped to the image (a clamped tap has weight 0 inside a chart)."""
    img = np.asarray(image, dtype=np.float64)
    H, W = img.shape[:2]
    tri = np.asarray(triangle, dtype=np.int64)
    hit = tri >= 0
    uvc = np.asarray(uv_corners, dtype=np.float64)[np.clip(tri, 0, None)]
    b = np.where(hit[:, None], np.asarray(bary, dtype=np.float64), 0.0)
    u = (b[:, 0] * uvc[:, 0, 0] + b[:, 1] * uvc[:, 1, 0]) + b[:, 2] * uvc[:, 2, 0]
    v = (b[:, 0] * uvc[:, 0, 1] + b[:, 1] * uvc[:, 1, 1]) + b[:, 2] * uvc[:, 2, 1]
    xs, ys, ws = bilinear_taps(u * W - 0.5, (1.0 - v) * H - 0.5)
    xs, ys = np.clip(xs, 0, W - 1), np.clip(ys, 0, H - 1)
    out = (img[ys, xs] * ws[..., None]).sum(axis=1)
    return np.where(hit[:, None], out, np.nan)
