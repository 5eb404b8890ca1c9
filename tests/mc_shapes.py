"""Analytic volumes and the on-surface property of a marching-cubes mesh: shared by tests/test_mc_oracle.py (the numpy
oracle) and tests/test_gpu_mcubes.py (the device kernels).  Not a test module."""
import numpy as np


def _grid(n, lo=-1.0, hi=1.0):
    ax = np.linspace(lo, hi, n, dtype=np.float32)
    return np.meshgrid(ax, ax, ax, indexing="ij")


def sphere(n, r=0.6, c=(0.05, -0.02, 0.03)):
    x, y, z = _grid(n)
    return (np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r).astype(np.float32)


def torus(n, R=0.55, r=0.22):
    x, y, z = _grid(n)
    return (np.sqrt((np.sqrt(x * x + y * y) - R) ** 2 + z * z) - r).astype(np.float32)


def check_on_surface(u, verts, threshold):
    """Each vertex lies on ONE grid edge, where the linear interpolant of the two samples equals the threshold."""
    base = np.floor(verts + 1e-12).astype(np.int64)
    frac = verts - base
    axis = np.argmax(frac, axis=1)
    assert ((frac > 0).sum(axis=1) <= 1).all(), "a vertex moves along one axis only"
    i0 = tuple(base.T)
    nb = base.copy()
    nb[np.arange(len(nb)), axis] += 1
    nb = np.minimum(nb, np.array(u.shape) - 1)
    f0, f1 = u[i0].astype(np.float64), u[tuple(nb.T)].astype(np.float64)
    t = frac[np.arange(len(frac)), axis]
    val = f0 + t * (f1 - f0)
    assert np.abs(val - threshold).max() < 1e-6
