"""Shared by tests/test_source_maps_host.py and tests/test_gpu_source_maps.py: the fixture of the reference's dataset
preparation (tests/golden/source_maps_small.npz, tools/gen_source_maps_golden.py), a float64 restatement of the closed
form that `rnb_gen_rays_*_from_maps` compute (include/rnbneus.h), and the light-equivalence check.

The reference's per-pixel lights are R u_k with a rotation R whose third column is the axis a = +-n/|n| (a_z >= 0) and
whose other two columns are whatever basis of the plane across a LAPACK's SVD returned, so lights can be compared with it
only up to a rotation about a.  `light_equivalence_error` takes that angle from light 0 and applies it to all lights: that
checks unit length, the slant, the spacing of the tilts, their cyclic order and the handedness at once."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "source_maps_small.npz")
# fewer than 25 fp32 roundings on values of magnitude <= 1, accumulated linearly: 25 x 2^-24 = 1.5e-6
LIGHT_BOUND = 2e-6
RGB_BOUND = 2e-6


def load_fixture():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}


def decode(values):
    """PNG values -> float64 values of the float32 numbers v / M"""
    return (values.astype(np.float32) / np.float32(np.iinfo(values.dtype).max)).astype(np.float64)


def decode_normals(values):
    c = (values.astype(np.float32) / np.float32(np.iinfo(values.dtype).max)) * np.float32(2.0) - np.float32(1.0)
    return c.astype(np.float64) * np.array([1.0, -1.0, -1.0])


def light_table(tilt_deg, slant_deg):
    """u_k = -(sin s cos t_k, sin s sin t_k, cos s), [L,3] float64"""
    t, s = np.radians(np.asarray(tilt_deg, dtype=np.float64)), np.radians(float(slant_deg))
    return -np.stack([np.sin(s) * np.cos(t), np.sin(s) * np.sin(t), np.cos(s) * np.ones_like(t)], axis=-1)


def axis_of(normals):
    """a = n/|n| flipped to a_z >= 0 ([...,3] float64)"""
    a = normals / np.linalg.norm(normals, axis=-1, keepdims=True)
    return np.where(a[..., 2:3] < 0, -a, a)


def closed_form(normals, albedo, rot, local, warm):
    """float64: normals [H,W,3] decoded, albedo [H,W,3] or None, rot [3,3] the view's rotation, local / warm [L,3].
    Returns images, images_warmup, light_directions (world) [L,H,W,3]."""
    a = axis_of(normals)
    q = -1.0 / (1.0 + a[..., 2])
    r = a[..., 0] * a[..., 1] * q
    b1 = np.stack([1.0 + a[..., 0] ** 2 * q, r, -a[..., 0]], axis=-1)
    b2 = np.stack([r, 1.0 + a[..., 1] ** 2 * q, -a[..., 1]], axis=-1)
    alb = np.ones_like(normals) if albedo is None else albedo
    l_cam = (local[:, None, None, 0:1] * b1[None] + local[:, None, None, 1:2] * b2[None] + local[:, None, None, 2:3] * a[None])
    shade = np.maximum((normals[None] * l_cam).sum(-1), 0.0)
    shade_w = np.maximum((normals[None] * warm[:, None, None, :]).sum(-1), 0.0)
    return alb[None] * shade[..., None], alb[None] * shade_w[..., None], l_cam @ rot.T


def light_equivalence_error(l_ref, l_test, axis):
    """l_ref, l_test [L,...,3], axis [...,3] (unit, the same space as the lights).  Per pixel: the angle about the axis
    that takes the reference's light 0 onto the tested light 0 (in the plane across the axis), then
    max_k |Rot(axis, angle) l_ref_k - l_test_k|.  Returns that maximum per pixel [...], float64."""
    l_ref, l_test, a = (np.asarray(v, dtype=np.float64) for v in (l_ref, l_test, axis))
    p_ref = l_ref[0] - (l_ref[0] * a).sum(-1, keepdims=True) * a
    p_test = l_test[0] - (l_test[0] * a).sum(-1, keepdims=True) * a
    theta = np.arctan2((a * np.cross(p_ref, p_test)).sum(-1), (p_ref * p_test).sum(-1))[None, ..., None]
    ab = np.broadcast_to(a, l_ref.shape)
    rotated = (l_ref * np.cos(theta) + np.cross(ab, l_ref) * np.sin(theta)
               + ab * (ab * l_ref).sum(-1, keepdims=True) * (1.0 - np.cos(theta)))
    return np.abs(rotated - l_test).max(axis=(0, -1))


def world_axis(normals, rot):
    """the reference's axis of every pixel in world space: decoded normals [...,3] (float64), rot [3,3]"""
    return axis_of(normals) @ rot.T
