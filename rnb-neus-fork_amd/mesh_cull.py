"""Mesh culling by the cameras, on the device: what the views of a masked multi-view reconstruction do not support is
removed from a mesh before it is evaluated, simplified or textured (csrc/mesh_cull.hip through `rnb_mesh_view_votes`,
csrc/mesh_clean.hip through `rnb_mesh_compact_triangles_*`, include/rnbneus.h).  Two kinds of geometry go: what lies
outside the visual hull of the masks (shells and blobs the masks never constrained, attached to the object or not), and
what no camera ever saw (interior shells, the closed underside on a turntable, caps at the bounding box).

The question is asked per VERTEX and per camera — in the frame? in the mask? unoccluded? — in ONE launch for all cameras
(`MeshIndex.view_votes`); `cull_mesh` turns the votes into a per-vertex keep, a per-triangle keep and a stable compaction.
include/rnbneus.h defines the status of a pair operation for operation and tests/mesh_cull_ref.py restates it in numpy:
device and numpy agree bit for bit, and the SEEN / OCCLUDED split is `MeshIndex.visible`'s.  There is no CPU path."""
from __future__ import annotations

import numpy as np
import torch

from . import native
from .mesh_clean import compact_triangles
from .mesh_args import check_points
from .mesh_raycast import VISIBLE_REL_TOL, index_device

STATUS_NAMES = ("out_of_frame", "outside_mask", "occluded", "seen")
RULES = ("all", "any")
CULL_KEYWORDS = ("rays", "views", "projections", "eyes", "masks", "image_size", "max_outside", "min_seen", "occlusion",
                 "dilate", "threshold", "rule")


def _host_matrices(who, name, m):
    """[C,4,4] float64 numpy from a [C,4,4] or [4,4] tensor or array"""
    a = m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
    a = np.asarray(a, dtype=np.float64)
    if a.shape == (4, 4):
        a = a[None]
    if a.ndim != 3 or a.shape[1:] != (4, 4):
        raise ValueError(f"{who}: {name} must be [C,4,4] or [4,4], got {a.shape}")
    return a


def camera_projections(intrinsics_inv, pose):
    """The world -> pixel projections and the eyes of cameras given as the ray generation holds them: `intrinsics_inv`
    (Kinv, pixel -> camera) and `pose` (camera -> world), [C,4,4] or [4,4], torch tensors or numpy arrays.  Returns
    `(P [C,3,4], eyes [C,3])`, float64 CPU tensors: P = inv(Kinv)[:3,:3] @ inv(pose)[:3,:4] and eyes = pose[:, :3, 3],
    computed on the host with numpy in float64.  A point o + s R Kinv (x, y, 1) of pixel (x, y)'s ray projects to (x, y)
    up to rounding: pixel centres sit at integer coordinates."""
    who = "camera_projections"
    kinv, pose = _host_matrices(who, "intrinsics_inv", intrinsics_inv), _host_matrices(who, "pose", pose)
    if kinv.shape[0] != pose.shape[0]:
        raise ValueError(f"{who}: {kinv.shape[0]} intrinsics but {pose.shape[0]} poses")
    if kinv.shape[0] == 0:
        return torch.zeros(0, 3, 4, dtype=torch.float64), torch.zeros(0, 3, dtype=torch.float64)
    P = np.linalg.inv(kinv)[:, :3, :3] @ np.linalg.inv(pose)[:, :3, :4]
    return torch.from_numpy(np.ascontiguousarray(P)), torch.from_numpy(np.ascontiguousarray(pose[:, :3, 3]))


def _check_mask_arguments(who, threshold, dilate):
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0.0 <= threshold <= 1.0:
        raise ValueError(f"{who}: threshold must be a number in [0, 1], not {threshold!r}")
    if isinstance(dilate, bool) or not isinstance(dilate, int) or dilate < 0:
        raise ValueError(f"{who}: dilate must be an integer >= 0, not {dilate!r}")


@torch.no_grad()
def binary_masks(masks, threshold=0.5, dilate=0):
    """[C,H,W] uint8 (1 inside, 0 outside) on the masks' device from a [C,H,W] or [C,H,W,Cm] stack: a pixel is set where
    channel 0 is > threshold x full scale — 255 for uint8, 65535 for uint16, 1 for a floating type: the reference's
    `masks > 0.5` on its images scaled to [0, 1].  `dilate=r` grows the set by a (2r + 1)^2 square (a torch max-pool; the
    image border does not wrap).  Works wherever the masks live."""
    who = "binary_masks"
    _check_mask_arguments(who, threshold, dilate)
    if not isinstance(masks, torch.Tensor) or masks.dim() not in (3, 4):
        raise ValueError(f"{who}: masks must be a [C,H,W] or [C,H,W,Cm] tensor, got "
                         f"{tuple(masks.shape) if isinstance(masks, torch.Tensor) else type(masks).__name__}")
    m = masks.detach()
    if m.dim() == 4:
        if m.shape[3] < 1:
            raise ValueError(f"{who}: masks {tuple(m.shape)} have no channel")
        m = m[..., 0]
    if m.dtype == torch.uint8:
        inside = m.to(torch.int32) > float(threshold) * 255.0
    elif m.dtype == torch.uint16:
        inside = m.to(torch.int32) > float(threshold) * 65535.0
    elif m.is_floating_point():
        inside = m > float(threshold)
    else:
        raise ValueError(f"{who}: masks must be uint8, uint16 or floating point, not {m.dtype}")
    out = inside.to(torch.uint8)
    if dilate > 0 and out.numel() > 0:
        k = 2 * int(dilate) + 1
        out = torch.nn.functional.max_pool2d(out[:, None].to(torch.float32), k, stride=1, padding=int(dilate))[:, 0].to(torch.uint8)
    return out.contiguous()


def _small(who, name, x, tail, dev):
    """a [C, *tail] float64 contiguous tensor on dev from a tensor or array"""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail or not (t.is_floating_point()):
        raise ValueError(f"{who}: {name} must be a float [C,{','.join(str(s) for s in tail)}] tensor, got {tuple(t.shape)} {t.dtype}")
    return t.detach().to(device=dev, dtype=torch.float64).contiguous()


def _check_size(who, image_size):
    if image_size is None:
        return None
    if (not isinstance(image_size, (tuple, list)) or len(image_size) != 2
            or any(isinstance(s, bool) or not isinstance(s, int) or s < 1 or s > 2 ** 31 - 1 for s in image_size)):
        raise ValueError(f"{who}: image_size must be (H, W), two positive integers, not {image_size!r}")
    return int(image_size[0]), int(image_size[1])


@torch.no_grad()
def view_votes(index, points, projections, eyes, masks=None, *, image_size=None, occlusion=True, rel_tol=VISIBLE_REL_TOL,
               return_status=False):
    """For every row of points [N,3] (float64 device tensor; float32 is widened exactly) and every camera: is it in the
    frame, in the mask, and not hidden by the mesh of `index`?  `projections` [C,3,4] and `eyes` [C,3] as
    `camera_projections` returns them (tensors anywhere, or arrays: they are small); `masks` [C,H,W] uint8 on the device
    (`binary_masks`) or None: then `image_size=(H, W)` gives the frame.  One launch for all cameras.
    Returns a dict of `out_of_frame`, `outside_mask`, `occluded`, `seen`, each [N] int32 — views of ONE [N,4] tensor,
    `counts`, whose rows sum to C — and with `return_status` also `status` [C,N] uint8 (0 .. 3 in that order).
    `occlusion=False` skips the segment cast: in frame and in mask is `seen`.  `rel_tol` as in `MeshIndex.visible`, whose
    answer for the segment eye -> point `seen` / `occluded` are.  include/rnbneus.h has the rule op for op.
    ValueError for wrong shapes / dtypes and for an index that does not cover its mesh (`covers == False`); RuntimeError
    for CPU points or masks, or another device.  No host synchronisation."""
    who = "MeshIndex.view_votes"
    check_points(who, "points", points)
    if isinstance(rel_tol, bool) or not isinstance(rel_tol, (int, float)) or not 0.0 <= rel_tol < 1.0:
        raise ValueError(f"{who}: rel_tol must be a number in [0, 1), not {rel_tol!r}")
    if not index.covers:
        raise ValueError(f"{who}: the index's grid does not cover its mesh (covers == False): build the index without grid=")
    size = _check_size(who, image_size)
    if masks is not None:
        if not isinstance(masks, torch.Tensor) or masks.dim() != 3 or masks.dtype != torch.uint8:
            raise ValueError(f"{who}: masks must be a [C,H,W] uint8 tensor (binary_masks makes one), got "
                             f"{(tuple(masks.shape), masks.dtype) if isinstance(masks, torch.Tensor) else type(masks).__name__}")
        if masks.shape[1] < 1 or masks.shape[2] < 1:
            raise ValueError(f"{who}: masks {tuple(masks.shape)} hold no pixel")
        if size is not None and size != (masks.shape[1], masks.shape[2]):
            raise ValueError(f"{who}: image_size {size} but masks of {tuple(masks.shape[1:])}")
        size = (int(masks.shape[1]), int(masks.shape[2]))
    if size is None:
        raise ValueError(f"{who}: without masks the frame is unknown: give image_size=(H, W)")
    dev = index_device(who, index, points, masks)
    P = _small(who, "projections", projections, (3, 4), dev)
    e = _small(who, "eyes", eyes, (3,), dev)
    n_cam = P.shape[0]
    if e.shape[0] != n_cam or (masks is not None and masks.shape[0] != n_cam):
        raise ValueError(f"{who}: {n_cam} projections, {e.shape[0]} eyes" + (f", {masks.shape[0]} masks" if masks is not None else ""))
    p = points.detach().to(torch.float64).contiguous()
    m = masks.detach().contiguous() if masks is not None else None
    N = p.shape[0]
    counts = torch.empty(N, 4, dtype=torch.int32, device=dev)
    status = torch.empty(n_cam, N, dtype=torch.uint8, device=dev) if return_status else None
    flags = native.MESH_BINS_COVER | (0 if occlusion else native.CULL_NO_OCCLUSION)
    if N > 0:
        with native.on_device(dev) as stream:
            native.check(native.load().rnb_mesh_view_votes(
                native.ptr(p), N, native.ptr(P), native.ptr(e), n_cam, native.ptr(m), size[0], size[1], *index.native_args(),
                float(rel_tol), flags, native.ptr(counts), native.ptr(status), stream))
    out = {name: counts[:, k] for k, name in enumerate(STATUS_NAMES)}
    out["counts"] = counts
    if return_status:
        out["status"] = status
    return out


def check_arguments(who, rays=None, views=None, projections=None, eyes=None, masks=None, image_size=None, max_outside=0,
                    min_seen=1, occlusion=True, dilate=0, threshold=0.5, rule="all"):
    """ValueError for `cull_mesh` keywords that contradict themselves (`cull_mesh`, the renderer's `cull=`)"""
    explicit = projections is not None or eyes is not None
    if rays is not None and (explicit or masks is not None or image_size is not None):
        raise ValueError(f"{who}: give the cameras and masks as rays= (a DeviceRays) or as projections=, eyes=, masks=, not both")
    if rays is None and not explicit:
        raise ValueError(f"{who}: no cameras: give rays= (a DeviceRays) or projections= and eyes=")
    if rays is None and (projections is None or eyes is None):
        raise ValueError(f"{who}: projections= and eyes= go together")
    if rays is not None and not all(hasattr(rays, k) for k in ("pose_all", "intrinsics_all_inv", "masks", "H", "W")):
        raise ValueError(f"{who}: rays must be a DeviceRays, not {type(rays).__name__}")
    if views is not None:
        if rays is None:
            raise ValueError(f"{who}: views= selects views of rays=; subset explicit cameras yourself")
        if isinstance(views, (str, bytes)) or any(isinstance(v, bool) or int(v) != v for v in views):
            raise ValueError(f"{who}: views must be a sequence of view indices, not {views!r}")
    _check_size(who, image_size)
    for name, x in (("max_outside", max_outside), ("min_seen", min_seen)):
        if isinstance(x, bool) or not isinstance(x, int) or x < 0:
            raise ValueError(f"{who}: {name} must be an integer >= 0, not {x!r}")
    if not isinstance(occlusion, bool):
        raise ValueError(f"{who}: occlusion must be a bool, not {occlusion!r}")
    _check_mask_arguments(who, threshold, dilate)
    if rule not in RULES:
        raise ValueError(f"{who}: rule must be one of {RULES}, not {rule!r}")


def _cameras_of(who, rays, views, threshold, dilate):
    """(P, eyes, binary masks [C,H,W] uint8) of a DeviceRays: its stored cameras, or with a refinement set the refined
    ones, as `view_rays` uses them"""
    n = int(rays.n_images)
    ids = list(range(n)) if views is None else [int(v) for v in views]
    if any(not 0 <= v < n for v in ids):
        raise IndexError(f"{who}: views {ids} out of range (n_images {n})")
    pose, kinv = rays.pose_all.detach(), rays.intrinsics_all_inv.detach()
    if getattr(rays, "_refinement", None) is not None and ids:
        poses, kinvs = [], []
        for v in ids:
            r_pose, r_kinv, _ = rays._camera(v)
            poses.append((pose[v] if r_pose is None else r_pose).detach().to(pose.device, torch.float32).reshape(4, 4))
            kinvs.append((kinv[v] if r_kinv is None else r_kinv).detach().to(kinv.device, torch.float32).reshape(4, 4))
        pose, kinv = torch.stack(poses), torch.stack(kinvs)
    else:
        sel = torch.as_tensor(ids, dtype=torch.int64, device=pose.device)
        pose, kinv = pose.index_select(0, sel), kinv.index_select(0, sel)
    P, eyes = camera_projections(kinv, pose)
    if views is None:
        bm = binary_masks(rays.masks, threshold, dilate)
    elif ids:       # view by view: slices of the stack in its own dtype, gathered once they are uint8
        bm = torch.cat([binary_masks(rays.masks[v:v + 1], threshold, dilate) for v in ids])
    else:
        bm = torch.zeros(0, int(rays.H), int(rays.W), dtype=torch.uint8, device=rays.masks.device)
    return P, eyes, bm


@torch.no_grad()
def cull_mesh(vertices, triangles, *, rays=None, views=None, projections=None, eyes=None, masks=None, image_size=None,
              max_outside=0, min_seen=1, occlusion=True, dilate=0, threshold=0.5, rule="all", attributes=None, index=None):
    """Removes from a mesh what the cameras do not support, on the device.  vertices [V,3] float64 in the cameras' world
    frame, triangles [T,3] int32 — device tensors.
    Cameras and masks: `rays=` a `DeviceRays` (its `pose_all`, `intrinsics_all_inv` and `masks`; `views=` a subset of its
    view indices; with `set_refinement` the refined cameras, as `view_rays` uses them), OR `projections=` [C,3,4] and
    `eyes=` [C,3] (`camera_projections`) with `masks=` ([C,H,W] or [C,H,W,Cm], any type `binary_masks` takes; None: no
    mask test, `image_size=(H, W)` gives the frame).  Giving both is a ValueError.  Masks go through
    `binary_masks(masks, threshold, dilate)` once.
    A VERTEX is kept when `outside_mask <= max_outside` and `seen >= min_seen` (votes of `MeshIndex.view_votes` over the
    cameras; with `occlusion=False` seen means in frame and in mask).  A TRIANGLE is kept when all of its corners are
    (`rule="all"`) or any is (`"any"`); the mesh is compacted to the kept triangles and the vertices they name
    (`mesh_clean.compact_triangles`), `attributes` (per-vertex device tensors) gathered with them.
    `index`: a `MeshIndex` of this mesh to cast at (one is built otherwise).
    Returns a dict shaped like `clean_mesh`'s: `vertices`, `triangles`, `attributes`, `vertex_index` [V'] int64,
    `triangle_index` [T'] int64 and `info`: the criteria, `n_cameras`, `votes` ([V,4] int32: out of frame, outside mask,
    occluded, seen), `keep_vertices` [V] bool, `n_vertices` / `n_triangles` as (before, after)."""
    who = "cull_mesh"
    check_arguments(who, rays, views, projections, eyes, masks, image_size, max_outside, min_seen, occlusion, dilate, threshold, rule)
    from .mesh_eval import MeshIndex
    if index is None:
        index = MeshIndex(vertices, triangles)
    elif index.n_vertices != vertices.shape[0] or index.n_triangles != triangles.shape[0]:
        raise ValueError(f"{who}: index holds {index.n_vertices} vertices / {index.n_triangles} triangles, the mesh "
                         f"{vertices.shape[0]} / {triangles.shape[0]}")
    dev = index.device
    if rays is not None:
        projections, eyes, bm = _cameras_of(who, rays, views, threshold, dilate)
        bm = bm.to(dev)
    else:
        if masks is not None and not isinstance(masks, torch.Tensor):
            masks = torch.as_tensor(np.asarray(masks))
        bm = binary_masks(masks.to(dev), threshold, dilate) if masks is not None else None
    votes = view_votes(index, vertices, projections, eyes, bm, image_size=image_size, occlusion=occlusion)
    keep_v = (votes["outside_mask"] <= int(max_outside)) & (votes["seen"] >= int(min_seen))
    V, T = vertices.shape[0], triangles.shape[0]
    if V > 0 and T > 0:
        corner = keep_v[triangles.detach().to(torch.int64).clamp(0, V - 1)]       # (an index out of range: dropped below)
        keep_t = corner.all(dim=1) if rule == "all" else corner.any(dim=1)
    else:
        keep_t = torch.zeros(T, dtype=torch.bool, device=dev)
    out = compact_triangles(vertices, triangles, keep_t, attributes)
    out["info"] = {"max_outside": int(max_outside), "min_seen": int(min_seen), "occlusion": occlusion, "dilate": int(dilate),
                   "threshold": float(threshold), "rule": rule, "n_cameras": int(projections.shape[0]),
                   "votes": votes["counts"], "keep_vertices": keep_v, "n_vertices": (V, out["vertices"].shape[0]),
                   "n_triangles": (T, out["triangles"].shape[0])}
    return out
