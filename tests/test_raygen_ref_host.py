"""tests/raygen_ref.py (the float32 restatement the GPU rays are held to bit for bit) against the oracle's
`gen_rays_at_view` on the `raygen_small` fixture, at the bounds tests/test_gpu_raygen.py holds the device to, and a check
that it really computes in float32.  No GPU."""
import numpy as np
import torch

from oracle import rnb_oracle as O
from tests import raygen_ref
from tests.golden_util import load_raygen


def _cases():
    ds, cases = load_raygen()
    for c in cases:
        v = int(c["img_idx"])
        yield ds, v, c["pixels_x"], c["pixels_y"]


def test_helper_is_the_oracles_arithmetic():
    n = 0
    for ds, v, px, py in _cases():
        ref = O.gen_rays_at_view(ds, v, px, py)
        rays_o, rays_d, near, far = (torch.from_numpy(a) for a in raygen_ref.pixel_rays(
            ds["intrinsics_all_inv"][v].numpy(), ds["pose_all"][v].numpy(), px.numpy(), py.numpy()))
        assert rays_o.dtype == torch.float32 and rays_d.shape == (px.numel(), 3) and near.shape == (px.numel(), 1)
        assert torch.equal(rays_o, ref["data"][:, :3])                       # a copy of the pose
        torch.testing.assert_close(rays_d, ref["data"][:, 3:6], rtol=0, atol=1e-6)
        torch.testing.assert_close(near, ref["near"], rtol=0, atol=2e-6)
        torch.testing.assert_close(far, ref["far"], rtol=0, atol=2e-6)
        n += px.numel()
    assert n > 0


def test_helper_computes_in_float32():
    """the same formula in float64, rounded once at the end, is a different set of bits: the helper's intermediate
    roundings are there"""
    differs = {"rays_d": False, "near": False, "far": False}
    for ds, v, px, py in _cases():
        args = (ds["intrinsics_all_inv"][v].numpy(), ds["pose_all"][v].numpy(), px.numpy(), py.numpy())
        f32 = raygen_ref.pixel_rays(*args)
        f64 = raygen_ref.pixel_rays(*args, dtype=np.float64)
        assert all(a.dtype == np.float64 for a in f64)
        assert np.array_equal(f32[0], f64[0].astype(np.float32))             # rays_o has no arithmetic
        for k, a, b in zip(("rays_d", "near", "far"), f32[1:], f64[1:]):
            differs[k] |= not np.array_equal(a, b.astype(np.float32))
            assert float(np.abs(a - b).max()) <= 2e-6, k                     # (and no further apart than roundings)
    assert all(differs.values()), differs
