"""Texture baking on the device: a per-triangle atlas of a (simplified) mesh, the field evaluated at its lattice samples,
and an albedo and an object-space normal image (csrc/texture_bake.hip through `rnb_texture_sample_points` /
`rnb_texture_pack`, include/rnbneus.h has the definition; the field evaluation is `NeuSRenderer.vertex_attributes`).

Every triangle gets a chart of the same size — vertex clustering leaves triangles of nearly one size — so a texel's
triangle and sample follow from its coordinates by integer arithmetic, and nothing is packed, counted or compacted.  A
sample on a shared edge is the same fp32 point from both triangles, so both sides of a seam evaluate the field at the
same place and no blending pass exists.  Device and numpy (tests/texture_bake_ref.py) agree bit for bit."""
from __future__ import annotations

import math
from dataclasses import asdict, dataclass

import numpy as np
import torch

from . import native, runtime
from .mesh_args import check_mesh

DEFAULT_CHART = 8
MAX_CHART = 255
GUARD = 5            # cell side = chart + GUARD


@dataclass(frozen=True)
class AtlasLayout:
    """`s` chart size (texel steps along a chart's legs), `c` = s + 5 the cell side, `cols` cells per row, `rows` cell rows
    in use, `W` x `H` the image, `samples_per_triangle` = (s + 1)(s + 2) / 2."""
    s: int
    c: int
    cols: int
    rows: int
    W: int
    H: int
    samples_per_triangle: int

    def asdict(self):
        return asdict(self)


def _int(who, name, x, lo, hi=None):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < lo or (hi is not None and x > hi):
        raise ValueError(f"{who}: {name} must be an integer >= {lo}" + (f" and <= {hi}" if hi is not None else "") + f", not {x!r}")
    return int(x)


def atlas_layout(n_triangles, size=None, chart=None) -> AtlasLayout:
    """The atlas of a mesh of `n_triangles` (host arithmetic only).  K = ceil(T / 2) cells of side c = chart + 5, two
    triangles per cell, row-major.
      `chart` alone: cols = ceil(sqrt(K)), rows = ceil(K / cols), W = cols c, H = rows c;
      `size`: a square size x size image, cols = size // c; ValueError when cols (size // c) < K;
      `size` alone: the largest chart that fits;  neither: chart = 8.
    ValueError for a chart outside [1, 255]."""
    who = "atlas_layout"
    T = _int(who, "n_triangles", n_triangles, 0, 2 ** 31 - 1)
    K = (T + 1) // 2
    if size is None:
        s = DEFAULT_CHART if chart is None else _int(who, "chart", chart, 1, MAX_CHART)
        c = s + GUARD
        cols = math.isqrt(K - 1) + 1 if K else 0
        rows = -(-K // cols) if cols else 0
        return AtlasLayout(s, c, cols, rows, cols * c, rows * c, (s + 1) * (s + 2) // 2)
    size = _int(who, "size", size, 1, 2 ** 15)
    for s in (range(MAX_CHART, 0, -1) if chart is None else [_int(who, "chart", chart, 1, MAX_CHART)]):
        c = s + GUARD
        cols = size // c
        if cols * cols >= K:
            return AtlasLayout(s, c, cols, -(-K // cols) if cols else 0, size, size, (s + 1) * (s + 2) // 2)
    raise ValueError(f"{who}: {T} triangles do not fit a {size} x {size} image" + (f" at chart = {chart}" if chart is not None else ""))


def atlas_uv(layout, n_triangles) -> np.ndarray:
    """[T,3,2] float64: (u, v) of every triangle corner, u = (x + 0.5) / W, v = 1 - (y + 0.5) / H with (x, y) the
    corner's texel.  Both halves of a cell have the same, mirrored orientation in UV (clockwise)."""
    T = _int("atlas_uv", "n_triangles", n_triangles, 0, 2 ** 31 - 1)
    if T == 0:
        return np.zeros((0, 3, 2), dtype=np.float64)
    s, c, cols = layout.s, layout.c, layout.cols
    if cols < 1 or cols * (layout.H // c) < (T + 1) // 2 or cols * c > layout.W:
        raise ValueError(f"atlas_uv: the layout does not hold {T} triangles")
    t = np.arange(T, dtype=np.int64)
    k = t // 2
    base = np.stack([(k % cols) * c, (k // cols) * c], axis=1)[:, None, :]
    lower = np.array([[1, 1], [1 + s, 1], [1, 1 + s]], dtype=np.int64)
    upper = np.array([[c - 2, c - 2], [c - 2 - s, c - 2], [c - 2, c - 2 - s]], dtype=np.int64)
    xy = (np.where((t % 2 == 1)[:, None, None], upper[None], lower[None]) + base).astype(np.float64)
    return np.stack([(xy[..., 0] + 0.5) / np.float64(layout.W), 1.0 - (xy[..., 1] + 0.5) / np.float64(layout.H)], axis=-1)


BAKE_KEYWORDS = ("size", "chart", "refine", "max_step", "threshold", "albedo", "slab", "chunk", "return_samples")


def check_arguments(who, size=None, chart=None, refine=0, max_step=None, threshold=0.0, albedo=None, slab=1 << 20,
                    chunk=65536, return_samples=False, need_max_step=True):
    """ValueError for bake keywords that cannot work, before anything is evaluated"""
    if size is not None:
        _int(who, "size", size, 1, 2 ** 15)
    if chart is not None:
        _int(who, "chart", chart, 1, MAX_CHART)
    if _int(who, "refine", refine, 0) > 0 and need_max_step and (max_step is None or not float(max_step) > 0.0):
        raise ValueError(f"{who}: refine > 0 needs max_step > 0 (model-space units)")
    if _int(who, "slab", slab, 64) % 64:
        raise ValueError(f"{who}: slab must be a positive multiple of 64, not {slab}")
    if _int(who, "chunk", chunk, 64) % 64:
        raise ValueError(f"{who}: chunk must be a positive multiple of 64, not {chunk}")


@torch.no_grad()
def bake_textures(renderer, vertices, triangles, *, size=None, chart=None, refine=0, max_step=None, threshold=0.0,
                  albedo=None, slab=1 << 20, chunk=65536, return_samples=False, to_host=True):
    """`NeuSRenderer.bake_textures`: see there."""
    who = "bake_textures"
    check_arguments(who, size, chart, refine, max_step, threshold, albedo, slab, chunk, return_samples)
    has_albedo = renderer.color_network is not None
    albedo = has_albedo if albedo is None else bool(albedo)
    if albedo and not has_albedo:
        raise ValueError(f"{who}: albedo=True on a renderer without an albedo network")
    if vertices is None:
        raise ValueError(f"{who}: vertices is None")
    check_mesh(who, triangles, None, vertices)
    T = triangles.shape[0]
    lay = atlas_layout(T, size, chart)
    n_s = lay.samples_per_triangle
    N = T * n_s
    if N >= 2 ** 31:
        raise ValueError(f"{who}: {T} triangles x {n_s} samples is not below 2^31: use a smaller chart")
    dev = native.gpu_device(triangles, vertices)
    vts, tri = vertices.detach().contiguous(), triangles.detach().contiguous()
    f32 = dict(dtype=torch.float32, device=dev)
    normal = torch.empty(N, 3, **f32)
    rgb = torch.empty(N, 3, dtype=torch.uint8, device=dev) if albedo else None
    keep = {}
    if return_samples:
        keep = {"points": torch.empty(N, 3, **f32), "sdf": torch.empty(N, 1, **f32)}
        if albedo:
            keep["albedo"] = torch.empty(N, renderer.desc.col_d_out, **f32)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    slabs = 0
    for first in range(0, N, slab):
        count = min(slab, N - first)
        pts = torch.empty(count, 3, **f32)
        runtime.texture_sample_points(vts, tri, lay.s, first, count, pts, bad)
        at = renderer.vertex_attributes(pts, refine=refine, max_step=max_step, threshold=threshold, albedo=albedo, chunk=chunk)
        normal[first:first + count] = at["normal"]
        if albedo:
            rgb[first:first + count] = at["rgb"]
        for k in keep:
            keep[k][first:first + count] = at[k]
        slabs += 1
    if lay.W * lay.H > 0:
        a_img, n_img, t_smp = runtime.texture_pack(vts, tri, lay.s, lay.cols, lay.W, lay.H, rgb, normal, albedo=albedo)
    else:
        a_img = torch.empty(0, 0, 4, dtype=torch.uint8, device=dev) if albedo else None
        n_img = torch.empty(0, 0, 4, dtype=torch.uint8, device=dev)
        t_smp = torch.empty(0, 0, dtype=torch.int32, device=dev)
    uv = atlas_uv(lay, T)
    out = {"uv": torch.from_numpy(uv).to(dev), "albedo_image": a_img, "normal_image": n_img, "texel_sample": t_smp}
    if return_samples:
        keep["normal"] = normal
        out.update(keep)
    if to_host:
        out = {k: (x.cpu().numpy() if isinstance(x, torch.Tensor) else x) for k, x in out.items()}
        out["uv"] = uv
    out["layout"] = lay
    out["info"] = {"samples": N, "bad_triangles": int(bad.cpu()), "slabs": slabs}     # (the call's one host read)
    return out


@torch.no_grad()
def sample_texture(image, uv_corners, triangle, bary):
    """What a ray hit sees of a texture: image [H,W,C] (or [H,W]) of any dtype, uv_corners [T,3,2] (`atlas_uv`), and the
    `triangle` [N] / `bary` [N,3] of `MeshIndex.raycast`.  uv = sum of bary x uv_corner, then a bilinear lookup with texel
    centres at (x + 0.5, y + 0.5), in float64: [N,C] (or [N]), NaN rows for misses (triangle < 0).  Inside a chart of the
    atlas every tap with a non-zero weight belongs to the hit triangle; taps are clamped to the image.  Torch ops only, on
    whatever device the tensors share; no host synchronisation."""
    who = "sample_texture"
    if not isinstance(image, torch.Tensor) or image.dim() not in (2, 3):
        raise ValueError(f"{who}: image must be a [H,W,C] or [H,W] tensor")
    if not isinstance(uv_corners, torch.Tensor) or uv_corners.dim() != 3 or tuple(uv_corners.shape[1:]) != (3, 2):
        raise ValueError(f"{who}: uv_corners must be a [T,3,2] tensor")
    if (not isinstance(triangle, torch.Tensor) or not isinstance(bary, torch.Tensor) or triangle.dim() != 1
            or tuple(bary.shape) != (triangle.shape[0], 3)):
        raise ValueError(f"{who}: needs triangle [N] and bary [N,3]")
    flat = image.dim() == 2
    img = image.detach().reshape(image.shape[0], image.shape[1], -1)
    H, W, Cn = img.shape
    N = triangle.shape[0]
    if N == 0 or uv_corners.shape[0] == 0 or H * W == 0:
        out = torch.full((N, Cn), float("nan"), dtype=torch.float64, device=img.device)
        return out[:, 0] if flat else out
    hit = triangle >= 0
    uvc = uv_corners.detach().to(torch.float64).index_select(0, triangle.clamp(min=0).to(torch.int64))
    b = torch.where(hit[:, None], bary.detach().to(torch.float64), torch.zeros((), dtype=torch.float64, device=bary.device))
    uv = (b[:, 0:1] * uvc[:, 0] + b[:, 1:2] * uvc[:, 1]) + b[:, 2:3] * uvc[:, 2]
    px, py = uv[:, 0] * W - 0.5, (1.0 - uv[:, 1]) * H - 0.5
    x0, y0 = torch.floor(px), torch.floor(py)
    fx, fy = (px - x0)[:, None], (py - y0)[:, None]
    x0, y0 = x0.to(torch.int64), y0.to(torch.int64)
    flat_img = img.reshape(H * W, Cn)

    def tap(dx, dy):
        x, y = (x0 + dx).clamp(0, W - 1), (y0 + dy).clamp(0, H - 1)
        return flat_img.index_select(0, y * W + x).to(torch.float64)

    out = (tap(0, 0) * ((1 - fx) * (1 - fy)) + tap(1, 0) * (fx * (1 - fy))) + (tap(0, 1) * ((1 - fx) * fy) + tap(1, 1) * (fx * fy))
    out = torch.where(hit[:, None], out, torch.full((), float("nan"), dtype=torch.float64, device=out.device))
    return out[:, 0] if flat else out
