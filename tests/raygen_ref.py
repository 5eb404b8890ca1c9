"""The ray arithmetic of csrc/raygen.hip (`pixel_ray`, `store_ray`) restated in numpy, operation by operation, so that
tests/test_gpu_raygen.py can hold the device's rays_o, rays_d, near and far to it bit for bit (tests/test_raygen_ref_host.py
holds this file to the oracle).  Every operation is one IEEE float32 operation on arrays: numpy never fuses a multiply
with an add, its float32 sqrt and division are correctly rounded, and the three-term sums are written out left to right
as the kernel writes them (the library is compiled without contraction).

    p = Kinv[:3,:3] (x, y, 1);  v = p / |p|;  rays_d = R v;  rays_o = t
    a = d.d;  bq = 2 (o.d);  mid = 0.5 (-bq) / a;  near / far = mid -+ 1
"""
import numpy as np


def _dot3(a, b):
    """a[0] b[0] + a[1] b[1] + a[2] b[2], accumulated left to right (a, b: sequences of three scalars or arrays)"""
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def pixel_rays(intrinsics_inv, pose, x, y, dtype=np.float32):
    """intrinsics_inv, pose [4,4], x, y [n] pixel coordinates (integer pixels or the float coordinates of a grid).
    Returns rays_o [n,3], rays_d [n,3], near [n,1], far [n,1] in `dtype`; float64 is only there to show what float32
    rounds away (the inputs are converted, the formula is the same)."""
    t = np.dtype(dtype).type
    kinv, pose = np.asarray(intrinsics_inv).astype(dtype), np.asarray(pose).astype(dtype)
    x, y = np.asarray(x).astype(dtype).reshape(-1), np.asarray(y).astype(dtype).reshape(-1)
    q = (x, y, t(1))
    p = [_dot3(kinv[r, :3], q) for r in range(3)]
    nrm = np.sqrt(_dot3(p, p))
    v = [p[0] / nrm, p[1] / nrm, p[2] / nrm]
    d = [_dot3(pose[r, :3], v) for r in range(3)]
    o = [np.full_like(x, pose[r, 3]) for r in range(3)]
    a = _dot3(d, d)
    bq = t(2) * _dot3(o, d)
    mid = t(0.5) * (-bq) / a
    out = np.stack(o, axis=-1), np.stack(d, axis=-1), (mid - t(1))[:, None], (mid + t(1))[:, None]
    assert all(r.dtype == np.dtype(dtype) for r in out)
    return out
