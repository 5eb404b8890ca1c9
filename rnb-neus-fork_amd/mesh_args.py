"""Argument checks the mesh tools share (mesh_clean, mesh_simplify, mesh_eval, mesh_raycast, mesh_cull, texture_bake): the
[V,3] float64 / [T,3] int32 mesh, [N,3] point arrays, per-vertex attributes, and the box of the finite vertices.  Every
check is a ValueError raised on the host before a device is looked at: the RuntimeError for CPU tensors
(`native.gpu_device`) comes after them in every public function."""
from __future__ import annotations

import torch


def _shape_of(x):
    return tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__


def check_mesh(who, triangles, n_vertices, vertices):
    """triangles [T,3] int32 and `vertices` [V,3] float64 (or, without them, `n_vertices`) as `marching_cubes` returns
    them, both counts within [0, 2^31 - 1]; returns V"""
    if not isinstance(triangles, torch.Tensor) or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError(f"{who}: triangles must be a [T,3] tensor, got {_shape_of(triangles)}")
    if triangles.dtype != torch.int32:
        raise ValueError(f"{who}: triangles must be int32 (what marching_cubes returns), not {triangles.dtype}")
    if vertices is not None:
        if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
            raise ValueError(f"{who}: vertices must be a [V,3] tensor, got {_shape_of(vertices)}")
        if vertices.dtype != torch.float64:
            raise ValueError(f"{who}: vertices must be float64 (what marching_cubes returns), not {vertices.dtype}")
        if n_vertices is not None and int(n_vertices) != vertices.shape[0]:
            raise ValueError(f"{who}: n_vertices = {n_vertices} but vertices has {vertices.shape[0]} rows")
        n_vertices = vertices.shape[0]
    if n_vertices is None:
        raise ValueError(f"{who}: give n_vertices or vertices")
    n_vertices = int(n_vertices)
    if n_vertices < 0 or n_vertices > 2 ** 31 - 1 or triangles.shape[0] > 2 ** 31 - 1:
        raise ValueError(f"{who}: {n_vertices} vertices / {triangles.shape[0]} triangles outside [0, 2^31 - 1]")
    return n_vertices


def check_points(who, name, x, dtypes=(torch.float64, torch.float32), noun="rays"):
    """x is a [N,3] tensor of one of `dtypes` (float64, with or without float32) with at most 2^31 - 1 rows"""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{who}: {name} must be a [N,3] tensor, got {_shape_of(x)}")
    if x.dtype not in dtypes:
        accepted = "(or float32, widened exactly)" if torch.float32 in dtypes else "(the mesh's own precision)"
        raise ValueError(f"{who}: {name} must be float64 {accepted}, not {x.dtype}")
    if x.shape[0] > 2 ** 31 - 1:
        raise ValueError(f"{who}: {x.shape[0]} {noun} outside [0, 2^31 - 1]")


def check_attributes(who, attributes, V):
    """the `attributes=` of a mesh tool as a dict (None: empty) of tensors with first dimension V"""
    attributes = dict(attributes or {})
    for name, a in attributes.items():
        if not isinstance(a, torch.Tensor) or a.dim() < 1 or a.shape[0] != V:
            raise ValueError(f"{who}: attribute {name!r} must be a tensor with first dimension V = {V}")
    return attributes


def finite_box(vertices):
    """(min [3], max [3]) over the vertices with all-finite coordinates, where they live and with no host read; (0, 0) when
    there is none (V = 0 included).  A non-finite vertex only ever belongs to triangles the mesh kernels skip."""
    ok = torch.isfinite(vertices).all(dim=1, keepdim=True)
    inf = torch.full_like(vertices, float("inf"))
    lo = torch.where(ok, vertices, inf).amin(dim=0) if vertices.shape[0] else inf.new_full((3,), float("inf"))
    hi = torch.where(ok, vertices, -inf).amax(dim=0) if vertices.shape[0] else inf.new_full((3,), float("-inf"))
    none = torch.isinf(lo)      # (a finite vertex makes all three finite: ±inf never passes `ok`)
    return torch.where(none, torch.zeros_like(lo), lo), torch.where(none, torch.zeros_like(hi), hi)
