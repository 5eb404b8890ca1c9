"""Mesh ray casting on the device: what a camera sees of a mesh — first hits, depth / normal / silhouette maps,
visibility, and the per-view angular error of normals (csrc/mesh_raycast.hip through `rnb_mesh_raycast`,
include/rnbneus.h).  Everything works on a `MeshIndex` (mesh_eval.py), whose bins and corners are already resident; the
methods `MeshIndex.raycast`, `.interpolate` and `.visible` are the functions below.  There is no CPU path.

A hit is `o + t d` with `d` as given (not normalised), the minimum over all triangles under (t as computed, triangle
index), by the watertight test of Woop, Benthin and Wald: bit-equal from run to run, and a closed surface has no
pinholes.  It is the same whatever the grid for every hit whose own point (sum of bary x corner) lies on its ray; a hit
on a triangle seen edge-on to within its size over 1024 scene sizes, a collinear zero-area one above all, is numerical
noise of the pair test that a one-cell grid reports and a finer one may not (include/rnbneus.h has the bound).
Gradients do not flow through a hit."""
from __future__ import annotations

import torch

from . import native
from .mesh_args import check_points

# `MeshIndex.visible`: the target point lies ON the mesh, so the segment eye -> point meets the point's own triangle (and
# its neighbours at an edge or a vertex) at t = 1 up to the rounding of the hit, a few 2^-52 of the scene's size over the
# segment's length.  1e-6 of the segment is far above that for any scene whose size is within 10^9 of its smallest
# eye-to-point distance, and far below the distance to a second surface that could hide the point.
VISIBLE_REL_TOL = 1e-6


def index_device(who, index, *tensors):
    """the GPU the given tensors share (`native.gpu_device`), which must be the mesh's"""
    dev = native.gpu_device(*tensors)
    if dev != index.device:
        raise RuntimeError(f"{who}: the rays live on {dev}, the mesh on {index.device}")
    return dev


def _check_bound(who, name, b, N):
    """a bound is None, a number, a one-element float tensor, or a float [N] (or [N,1]) tensor"""
    if isinstance(b, torch.Tensor):
        per_ray = b.dim() == 1 or (b.dim() == 2 and b.shape[1] == 1)
        if b.dtype not in (torch.float64, torch.float32) or not (b.numel() == 1 or (b.numel() == N and per_ray)):
            raise ValueError(f"{who}: {name} must be a scalar or a float [N] tensor, got {tuple(b.shape)} {b.dtype}")
    elif b is not None and (isinstance(b, bool) or not isinstance(b, (int, float))):
        raise ValueError(f"{who}: {name} must be a scalar or a float [N] tensor, not {type(b).__name__}")


def _bound(who, name, b, N, dev):
    """a checked bound as the library reads it: None, or a contiguous [N] float64 tensor on the device"""
    if b is None:
        return None
    if isinstance(b, torch.Tensor):
        if not b.is_cuda:
            raise RuntimeError(native.NO_CPU_PATH)
        if b.device != dev:
            raise RuntimeError(f"{who}: {name} lives on {b.device}, the rays on {dev}")
        return b.detach().to(torch.float64).reshape(-1).expand(N).contiguous()
    return torch.full((N,), float(b), dtype=torch.float64, device=dev)


def _cast(who, index, origins, directions, t_min, t_max, want_bary=True):
    """the checks and the launch: (o, d as float64, t [N], triangle [N], bary [N,3] or None)"""
    check_points(who, "origins", origins)
    check_points(who, "directions", directions)
    if origins.shape != directions.shape:
        raise ValueError(f"{who}: origins {tuple(origins.shape)} and directions {tuple(directions.shape)} differ in shape")
    if not index.covers:
        raise ValueError(f"{who}: the index's grid does not cover its mesh (covers == False): build the index without grid=")
    N = origins.shape[0]
    _check_bound(who, "t_min", t_min, N)
    _check_bound(who, "t_max", t_max, N)
    dev = index_device(who, index, origins, directions)
    o = origins.detach().to(torch.float64).contiguous()
    d = directions.detach().to(torch.float64).contiguous()
    lo, hi = _bound(who, "t_min", t_min, N, dev), _bound(who, "t_max", t_max, N, dev)
    t = torch.empty(N, dtype=torch.float64, device=dev)
    tri = torch.empty(N, dtype=torch.int32, device=dev)
    bary = torch.empty(N, 3, dtype=torch.float64, device=dev) if want_bary else None
    if N > 0:
        with native.on_device(dev) as stream:
            native.check(native.load().rnb_mesh_raycast(
                native.ptr(o), native.ptr(d), native.ptr(lo), native.ptr(hi), N, *index.native_args(),
                native.MESH_BINS_COVER, native.ptr(t), native.ptr(tri), native.ptr(bary), stream))
    return o, d, t, tri, bary


@torch.no_grad()
def raycast(index, origins, directions, t_min=None, t_max=None):
    """The first hit of every ray `origins + t directions` ([N,3] float64 device tensors; float32 is widened exactly)
    with the mesh of `index`, t_min <= t <= t_max (scalars or [N]; None: 0 and +inf).  Returns a dict of device tensors:
    `t` [N] float64, `triangle` [N] int32, `bary` [N,3] float64 (the weights of the triangle's three corners), `hit` [N]
    bool, `point` [N,3] = o + t d, `normal` [N,3] (the unit face normal (b - a) x (c - a) / |.|).  No hit: t = +inf,
    triangle = -1, NaN elsewhere.  A ray with a non-finite origin or direction, a zero direction or a NaN bound: t = NaN.
    The rays are cast in the order given: sorting 10^6 shuffled segments by the cell of their origin, as `closest` sorts
    its queries, gained nothing (profiles/mesh_raycast_bench.txt).
    ValueError for wrong shapes / dtypes and for an index that does not cover its mesh (`covers == False`: build the
    index without grid=); RuntimeError for CPU tensors or another device.  No host synchronisation."""
    o, d, t, tri, bary = _cast("MeshIndex.raycast", index, origins, directions, t_min, t_max)
    dev, N = t.device, t.shape[0]
    hit = tri >= 0
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    point = torch.where(hit[:, None], o + t[:, None] * d, nan)
    if index.n_triangles > 0:
        c = index.corners.index_select(0, tri.clamp(min=0).to(torch.int64))
        n = torch.linalg.cross(c[:, 3:6] - c[:, 0:3], c[:, 6:9] - c[:, 0:3])
        normal = torch.where(hit[:, None], n / torch.linalg.norm(n, dim=1, keepdim=True), nan)
    else:
        normal = nan.expand(N, 3).clone()
    return {"t": t, "triangle": tri, "bary": bary, "hit": hit, "point": point, "normal": normal}


def _check_hits(who, hits):
    if not isinstance(hits, dict) or not {"triangle", "bary"} <= set(hits):
        raise ValueError(f"{who}: hits must be the dict MeshIndex.raycast returns")
    tri, bary = hits["triangle"], hits["bary"]
    if (not isinstance(tri, torch.Tensor) or not isinstance(bary, torch.Tensor) or tri.dim() != 1
            or bary.shape != (tri.shape[0], 3) or tri.dtype not in (torch.int32, torch.int64) or not bary.is_floating_point()):
        raise ValueError(f"{who}: hits needs triangle [N] int32 and bary [N,3] float")
    return tri, bary


@torch.no_grad()
def interpolate(index, hits, vertex_values):
    """Per-vertex values [V,C] (or [V]) interpolated barycentrically at the hits of `raycast`: [N,C] (or [N]) in the
    values' floating dtype (float64 for integer values), NaN rows for misses.  Torch gathers only; works wherever the
    tensors live (an index may be any object with `triangles` and `n_vertices`)."""
    who = "MeshIndex.interpolate"
    tri, bary = _check_hits(who, hits)
    vals = vertex_values
    if not isinstance(vals, torch.Tensor) or vals.dim() not in (1, 2) or vals.shape[0] != index.n_vertices:
        raise ValueError(f"{who}: vertex_values must be a [V,C] or [V] tensor with V = {index.n_vertices}, got "
                         f"{tuple(vals.shape) if isinstance(vals, torch.Tensor) else type(vals).__name__}")
    if vals.device != tri.device or index.triangles.device != tri.device:
        raise RuntimeError(f"{who}: the hits, the values and the mesh live on different devices")
    flat = vals.dim() == 1
    v = vals.detach().reshape(vals.shape[0], -1)
    v = v if v.is_floating_point() else v.to(torch.float64)
    hit = tri >= 0
    out = torch.full((tri.shape[0], v.shape[1]), float("nan"), dtype=v.dtype, device=v.device)
    if index.triangles.shape[0] > 0 and tri.shape[0] > 0:
        idx = index.triangles.index_select(0, tri.clamp(min=0).to(torch.int64)).to(torch.int64)       # [N,3]
        w = torch.where(hit[:, None], bary, torch.zeros_like(bary)).to(v.dtype)
        acc = (w[:, 0:1] * v.index_select(0, idx[:, 0]) + w[:, 1:2] * v.index_select(0, idx[:, 1])) + w[:, 2:3] * v.index_select(0, idx[:, 2])
        out = torch.where(hit[:, None], acc, out)
    return out[:, 0] if flat else out


@torch.no_grad()
def visible(index, points, eye, rel_tol=VISIBLE_REL_TOL):
    """bool [N]: the segment from `eye` ([3] or [N,3]) to each row of points [N,3] meets no triangle at a parameter
    t in [0, 1 - rel_tol) (t = 0 at the eye, 1 at the point).  The point itself lies on the mesh, so its own triangle is
    met at t = 1 up to rounding: `rel_tol` (default 1e-6 of the segment, see VISIBLE_REL_TOL) keeps that hit from hiding
    it.  A point with a non-finite coordinate, or equal to its eye, is not visible.  No host synchronisation."""
    who = "MeshIndex.visible"
    check_points(who, "points", points)
    if not isinstance(eye, torch.Tensor) or eye.dtype not in (torch.float64, torch.float32) or (
            tuple(eye.shape) != (3,) and eye.shape != points.shape):
        raise ValueError(f"{who}: eye must be a float [3] or [N,3] tensor")
    if isinstance(rel_tol, bool) or not isinstance(rel_tol, (int, float)) or not 0.0 <= rel_tol < 1.0:
        raise ValueError(f"{who}: rel_tol must be a number in [0, 1), not {rel_tol!r}")
    index_device(who, index, points, eye)
    p = points.detach().to(torch.float64)
    e = eye.detach().to(torch.float64).expand_as(p).contiguous()
    t = _cast(who, index, e, p - e, 0.0, 1.0, want_bary=False)[2]           # only t: no point, normal or bary is built
    return t >= 1.0 - float(rel_tol)                  # +inf: nothing met; NaN (an unusable segment): not visible


@torch.no_grad()
def mesh_view_maps(index, rays_o, rays_d=None, shape=None, vertex_normals=None, vertex_albedo=None):
    """The maps of one view of a mesh.  `rays_o`, `rays_d` [n,3] (float32 or float64), or the dict of
    `DeviceRays.view_rays(...)` in place of `rays_o` (its `H`, `W` give `shape` unless one is given).  Returns a dict of
    device tensors: `mask` [n] bool (the silhouette), `depth` [n] float64 (the distance along the UNIT direction,
    t |d|; +inf off the mesh), `face_normal` [n,3], `triangle` [n] int32, `bary` [n,3] and, where the per-vertex arrays
    are given ([V,3], e.g. from `vertex_attributes`), `normal` (interpolated and re-normalised) and `albedo`
    (interpolated); NaN off the mesh.  With `shape = (H, W)` every map is reshaped to [H, W, ...]."""
    who = "mesh_view_maps"
    if isinstance(rays_o, dict):
        rays = rays_o
        if rays_d is not None:
            raise ValueError(f"{who}: give the dict of view_rays or rays_o and rays_d, not both")
        if not {"rays_o", "rays_d"} <= set(rays):
            raise ValueError(f"{who}: the dict must hold rays_o and rays_d, as DeviceRays.view_rays returns them")
        rays_o, rays_d = rays["rays_o"], rays["rays_d"]
    else:
        rays = {}
    if rays_d is None:
        raise ValueError(f"{who}: rays_d is missing")
    check_points(who, "rays_o", rays_o)
    check_points(who, "rays_d", rays_d)
    if shape is None and "H" in rays and "W" in rays and rays_o.shape[0] == int(rays["H"]) * int(rays["W"]):
        shape = (int(rays["H"]), int(rays["W"]))
    if shape is not None:
        if not isinstance(shape, (tuple, list)) or len(shape) != 2 or any(isinstance(s, bool) or not isinstance(s, int) for s in shape):
            raise ValueError(f"{who}: shape must be (H, W), two integers, not {shape!r}")
        shape = tuple(int(s) for s in shape)
        if len(shape) != 2 or shape[0] * shape[1] != rays_o.shape[0]:
            raise ValueError(f"{who}: shape {shape} does not hold {rays_o.shape[0]} rays")
    hits = raycast(index, rays_o, rays_d)
    length = torch.linalg.norm(rays_d.detach().to(torch.float64), dim=1)
    out = {"mask": hits["hit"], "depth": torch.where(hits["hit"], hits["t"] * length, hits["t"]),
           "face_normal": hits["normal"], "triangle": hits["triangle"], "bary": hits["bary"]}
    if vertex_normals is not None:
        n = interpolate(index, hits, vertex_normals)
        out["normal"] = n / torch.linalg.norm(n, dim=1, keepdim=True)
    if vertex_albedo is not None:
        out["albedo"] = interpolate(index, hits, vertex_albedo)
    if shape is not None:
        out = {k: v.reshape(shape + tuple(v.shape[1:])) for k, v in out.items()}
    return out


def angular_error_statistics(n_a, n_b, mask=None):
    """ONE tensor [4] float64 where the normals live: mean, median, rms of the angle between n_a and n_b in degrees and
    the pixel count, over the pixels where the mask holds and both normals are finite and non-zero.  Torch reductions
    only, no synchronisation.  The angle is atan2(|a x b|, a . b): exact near 0 and 180 degrees, where acos loses half
    the digits; the normals need not be unit.  NaN statistics and count 0 when no pixel qualifies."""
    who = "normal_angular_error"
    if not isinstance(n_a, torch.Tensor) or not isinstance(n_b, torch.Tensor) or n_a.shape != n_b.shape or n_a.dim() < 1 or n_a.shape[-1] != 3:
        raise ValueError(f"{who}: n_a and n_b must be [...,3] tensors of one shape")
    if not n_a.is_floating_point() or not n_b.is_floating_point():
        raise ValueError(f"{who}: n_a and n_b must be floating-point tensors")
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.numel() != n_a.numel() // 3):
        raise ValueError(f"{who}: mask must hold one value per normal")
    a, b = n_a.detach().to(torch.float64).reshape(-1, 3), n_b.detach().to(torch.float64).reshape(-1, 3)
    # the cross product with every product rounded on its own: a x a is then exactly zero, and a map against itself 0
    ax, ay, az, bx, by, bz = a[:, 0], a[:, 1], a[:, 2], b[:, 0], b[:, 1], b[:, 2]
    cross = torch.sqrt((ay * bz - az * by) ** 2 + (az * bx - ax * bz) ** 2 + (ax * by - ay * bx) ** 2)
    dot = (a * b).sum(dim=1)
    ok = torch.isfinite(a).all(dim=1) & torch.isfinite(b).all(dim=1) & ((cross > 0) | (dot != 0))
    if mask is not None:
        ok = ok & (mask.reshape(-1) != 0).to(ok.device)
    ang = torch.rad2deg(torch.atan2(cross, dot))
    count = ok.sum()
    n = count.clamp(min=1).to(torch.float64)
    kept = torch.where(ok, ang, torch.zeros_like(ang))
    mean, rms = kept.sum() / n, torch.sqrt((kept * kept).sum() / n)
    # the median of the kept angles without a data-dependent shape: the others sort to the end as +inf
    srt = torch.sort(torch.where(ok, ang, torch.full_like(ang, float("inf")))).values
    if srt.numel() > 0:
        # a gather with a device index: indexing with a 0-dim tensor would read it on the host
        mid = torch.stack([(count - 1).clamp(min=0) // 2, (count.clamp(min=1) // 2).clamp(max=srt.numel() - 1)])
        pair = srt.gather(0, mid)
        median = 0.5 * (pair[0] + pair[1])
    else:
        median = torch.zeros((), dtype=torch.float64, device=a.device)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=a.device)
    stats = torch.stack([mean, median, rms])
    return torch.cat([torch.where(count > 0, stats, nan), count.to(torch.float64).reshape(1)])


@torch.no_grad()
def normal_angular_error(n_a, n_b, mask=None):
    """The per-view angular error of normals: `mean`, `median`, `rms` of the angle between n_a and n_b ([...,3], e.g. a
    `mesh_view_maps` normal map against the input normal map, in one frame) in degrees, and `count`, over the pixels
    where `mask` (None: everywhere) holds and both normals are finite and non-zero.  Torch reductions gathered into one
    tensor, read with ONE host synchronisation (`angular_error_statistics` is that tensor)."""
    s = angular_error_statistics(n_a, n_b, mask).cpu().tolist()
    return {"mean": s[0], "median": s[1], "rms": s[2], "count": int(s[3])}
