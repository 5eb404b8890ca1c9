"""fp64 numpy reference of the mesh culling (csrc/mesh_cull.hip, rnb_mesh_view_votes in include/rnbneus.h): the status of
every (camera, point) pair in the header's operation order, the votes, the compaction by a per-triangle keep and
`cull_mesh`'s rule, and the scene the tests share.  Not a test module.

numpy rounds every product and sum on its own and the kernel is compiled without contraction, so device and reference are
required to agree BIT FOR BIT.  Step 3, the segment cast, is tests/mesh_raycast_ref.py's brute-force `raycast_all` (the
pair test `ray_triangle` over ALL triangles)."""
import numpy as np

from tests.mesh_raycast_ref import icosphere, raycast_all

OUT_OF_FRAME, OUTSIDE_MASK, OCCLUDED, SEEN = 0, 1, 2, 3
REL_TOL = 1e-6


def project(points, P):
    """(x, y, w) [N] of points [N,3] under one projection P [3,4]: ((P0 X + P1 Y) + P2 Z) + P3 per row"""
    X, Y, Z = points[:, 0], points[:, 1], points[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return tuple(((P[r, 0] * X + P[r, 1] * Y) + P[r, 2] * Z) + P[r, 3] for r in range(3))


def frame_status(points, P, mask, H, W):
    """steps 1 and 2 for one camera: (reaches [N] bool: the pair goes on to step 3, status [N] uint8 for the others, px, py)"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    x, y, w = project(points, np.asarray(P, dtype=np.float64))
    ok = np.isfinite(points).all(axis=1) & np.isfinite(w) & (w > 0.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        a, b = x / w + 0.5, y / w + 0.5
        inside = ok & (a >= 0.0) & (a < float(W)) & (b >= 0.0) & (b < float(H))
    px = np.where(inside, np.floor(np.where(inside, a, 0.0)), 0).astype(np.int64)
    py = np.where(inside, np.floor(np.where(inside, b, 0.0)), 0).astype(np.int64)
    status = np.full(len(points), OUT_OF_FRAME, dtype=np.uint8)
    reaches = inside.copy()
    if mask is not None:
        off = inside & (np.asarray(mask)[py, px] == 0)
        status[off] = OUTSIDE_MASK
        reaches &= ~off
    return reaches, status, px, py


def view_votes(points, projections, eyes, masks, size, vertices, triangles, occlusion=True, rel_tol=REL_TOL):
    """(status [C,N] uint8, counts [N,4] int32) of the rule of include/rnbneus.h; masks [C,H,W] or None, size = (H, W)"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    P, eyes = np.asarray(projections, dtype=np.float64).reshape(-1, 3, 4), np.asarray(eyes, dtype=np.float64).reshape(-1, 3)
    C, N = len(P), len(points)
    H, W = size
    status = np.zeros((C, N), dtype=np.uint8)
    for c in range(C):
        reaches, st, _, _ = frame_status(points, P[c], None if masks is None else masks[c], H, W)
        if occlusion and reaches.any():
            ids = np.flatnonzero(reaches)
            o = np.tile(eyes[c], (len(ids), 1))
            with np.errstate(invalid="ignore", over="ignore"):
                d = points[ids] - o
            t = raycast_all(o, d, vertices, triangles, 0.0, 1.0)[0]
            with np.errstate(invalid="ignore"):
                st[ids] = np.where(t >= 1.0 - rel_tol, SEEN, OCCLUDED)
        else:
            st[reaches] = SEEN
        status[c] = st
    counts = np.stack([(status == k).sum(axis=0) for k in range(4)], axis=1).astype(np.int32).reshape(N, 4)
    return status, counts


def compact_triangles(vertices, triangles, keep):
    """(vertices', triangles', vertex_index int64, triangle_index int64): the triangles keep selects whose indices are in
    range, the vertices they name, stable, indices remapped"""
    v, t = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    V = len(v)
    kept = (np.asarray(keep).reshape(-1) != 0) & ((t >= 0) & (t < V)).all(axis=1)
    t_index = np.flatnonzero(kept).astype(np.int64)
    used = np.zeros(V, dtype=bool)
    used[t[kept].reshape(-1)] = True
    v_index = np.flatnonzero(used).astype(np.int64)
    new = np.full(V, -1, dtype=np.int32)
    new[v_index] = np.arange(len(v_index), dtype=np.int32)
    return v[v_index], new[t[kept]].reshape(-1, 3).astype(np.int32), v_index, t_index


def cull(vertices, triangles, projections, eyes, masks, size, max_outside=0, min_seen=1, occlusion=True, rule="all"):
    """`cull_mesh` on binary masks: (vertices', triangles', vertex_index, triangle_index, counts [V,4])"""
    v, t = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    counts = view_votes(v, projections, eyes, masks, size, v, t, occlusion)[1]
    keep_v = (counts[:, OUTSIDE_MASK] <= max_outside) & (counts[:, SEEN] >= min_seen)
    corner = keep_v[np.clip(t, 0, max(len(v) - 1, 0))] if len(v) else np.zeros((len(t), 3), dtype=bool)
    keep_t = corner.all(axis=1) if rule == "all" else corner.any(axis=1)
    return compact_triangles(v, t, keep_t) + (counts,)


# ---- the shared scene (callers must not modify it) ------------------------------------------------------------------------

H = W = 48
FOCAL, CENTRE, DISTANCE = 60.0, 23.5, 3.0
N_OUTER, N_INNER, N_FLOATER = 642, 162, 12
_SCENE = {}


def look_at_pose(eye):
    """camera-to-world [4,4] of a camera at `eye` looking at the origin: columns x (right), y (down), z (forward)"""
    eye = np.asarray(eye, dtype=np.float64)
    fwd = -eye / np.linalg.norm(eye)
    helper = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    right = np.cross(fwd, helper)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, down, fwd, eye
    return pose


def scene():
    """An outer unit icosphere(3) (642 / 1280), an inner icosphere(2) scaled by 0.5 with reversed winding (162 / 320), a
    floater icosphere(0) scaled by 0.08 at (1.25, 0.3, -0.2) (12 / 20); six cameras on the +-axes at distance 3 looking at
    the origin, 48 x 48, focal 60 px, principal point 23.5; masks = the disc of radius 60 tan(asin(1.03 / 3)) px about the
    principal point.  A dict: vertices, triangles, intrinsics_inv, pose [6,4,4], projections [6,3,4], eyes [6,3], masks
    [6,48,48] uint8, size, and the reference's `status` / `counts` with the masks (and `counts_nomask`, `counts_noocc`)."""
    if not _SCENE:
        vo, to = icosphere(3)
        vi, ti = icosphere(2)
        vf, tf = icosphere(0)
        assert (len(vo), len(to), len(vi), len(ti), len(vf), len(tf)) == (642, 1280, 162, 320, 12, 20)
        v = np.concatenate([vo, 0.5 * vi, 0.08 * vf + np.array([1.25, 0.3, -0.2])])
        t = np.concatenate([to, ti[:, ::-1] + len(vo), tf + len(vo) + len(vi)]).astype(np.int32)
        eyes = DISTANCE * np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
        pose = np.stack([look_at_pose(e) for e in eyes])
        K = np.array([[FOCAL, 0.0, CENTRE, 0.0], [0.0, FOCAL, CENTRE, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
        kinv = np.tile(np.linalg.inv(K), (6, 1, 1))
        P = K[:3, :3][None] @ np.linalg.inv(pose)[:, :3, :4]
        r = FOCAL * np.tan(np.arcsin(1.03 / DISTANCE))
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        disc = (((xs - CENTRE) ** 2 + (ys - CENTRE) ** 2) <= r * r).astype(np.uint8)
        masks = np.ascontiguousarray(np.tile(disc, (6, 1, 1)))
        s = {"vertices": np.ascontiguousarray(v), "triangles": np.ascontiguousarray(t), "intrinsics_inv": kinv, "pose": pose,
             "projections": np.ascontiguousarray(P), "eyes": np.ascontiguousarray(pose[:, :3, 3]), "masks": masks, "size": (H, W)}
        s["status"], s["counts"] = view_votes(v, P, s["eyes"], masks, (H, W), v, t)
        s["counts_nomask"] = view_votes(v, P, s["eyes"], None, (H, W), v, t)[1]
        s["counts_noocc"] = view_votes(v, P, s["eyes"], masks, (H, W), v, t, occlusion=False)[1]
        _SCENE.update(s)
    return _SCENE
