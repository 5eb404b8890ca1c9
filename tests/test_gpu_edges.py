"""GPU edge cases of the renderer interface: ragged and tiny ray counts, a large batch (max size the bench
shape is sharded from), shard consistency (the property the data-parallel split relies on), the SDF grid query
of extract_fields and an empty batch.  Tolerances as in test_gpu_parity.py's point-wise tests."""
import numpy as np
import pytest
import torch

from oracle import rnb_oracle as O
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device

pytestmark = pytest.mark.gpu


def _tiny(R, seed=0):
    mc = O.ModelConf(sdf=O.SDFConf(d_out=65, d_hidden=64), color=O.ColorConf(d_feature=64, d_hidden=64),
                     render=O.RenderConf(n_samples=16, n_importance=16))
    torch.manual_seed(seed)
    p = O.init_params(mc)
    with torch.no_grad():
        p["dev.variance"].fill_(0.4)
    return mc, p, R.build_from_named_params(mc, p, device())


@pytest.mark.parametrize("B", [1, 3, 37, 129])
def test_ragged_ray_counts_match_oracle(R, B):
    """Ray counts that are not a multiple of any tile size (points are padded to 128 internally)."""
    mc, p, (sdf, dev, col, ren) = _tiny(R)
    batch = O.synthetic_batch(B, seed=11, step=B)
    b = {k: v.to(device()) for k, v in batch.items()}
    out = ren.render_rnb(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=0.7,
                         t_rand=b["t_rand"])
    assert out["color_fine"].shape == (3, B, 3) and out["weights"].shape == (B, 32)
    loss = O.rnb_loss(out, b["true_rgb"], b["mask"])[0]
    loss.backward()
    z = ren.last_z_vals.cpu()
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    ref = O.render_rnb(pr, mc, batch["rays_o"], batch["rays_d"], batch["near"], batch["far"], batch["lights_dir"],
                       cos_anneal_ratio=0.7, z_vals=z)
    O.rnb_loss(ref, batch["true_rgb"], batch["mask"])[0].backward()
    for k in ("color_fine", "weights", "weight_sum", "gradients", "cdf_fine", "gradient_error"):
        torch.testing.assert_close(out[k].detach().cpu(), ref[k].detach(), rtol=1e-4, atol=2e-5,
                                   msg=lambda m: f"{k}: {m}")
    for name, leaf in (("sdf.lin1.weight_v", sdf.lin1.weight_v), ("sdf.lin8.bias", sdf.lin8.bias),
                       ("color.lin0.weight_v", col.lin0.weight_v), ("dev.variance", dev.variance)):
        g, gr = leaf.grad.cpu().double(), pr[name].grad.double()
        assert float((g - gr).norm()) <= 2e-3 * float(gr.norm()) + 1e-7, name


def test_shards_of_a_batch_render_like_the_whole_batch(R):
    """Rays are independent: rendering two halves of a batch on given depths reproduces the whole batch
    (what parallel.shard_batch relies on); 4096 rays = the largest per-GPU batch of BASELINE's configs."""
    mc, p, (sdf, dev, col, ren) = _tiny(R, seed=2)
    batch = O.synthetic_batch(4096, seed=13, step=1)
    b = {k: v.to(device()) for k, v in batch.items()}
    with torch.no_grad():
        whole = ren.render_rnb(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=1.0,
                               t_rand=b["t_rand"])
        z = ren.last_z_vals
        parts = []
        for lo, hi in ((0, 1000), (1000, 4096)):        # deliberately ragged split
            parts.append(ren.render_rnb(b["rays_o"][lo:hi], b["rays_d"][lo:hi], b["near"][lo:hi], b["far"][lo:hi],
                                        b["lights_dir"][:, lo:hi], cos_anneal_ratio=1.0, t_rand=b["t_rand"][lo:hi]))
            assert torch.equal(ren.last_z_vals, z[lo:hi])   # sampling is per ray: bit-identical depths
    assert whole["weights"].shape == (4096, 32)
    torch.testing.assert_close(torch.cat([q["weights"] for q in parts]), whole["weights"], rtol=0, atol=0)
    torch.testing.assert_close(torch.cat([q["color_fine"] for q in parts], dim=1), whole["color_fine"], rtol=0, atol=0)
    assert bool(torch.isfinite(whole["color_fine"]).all())


def test_extract_fields_matches_oracle_grid(R):
    """models/renderer.py:10-25 / :1219-1224: -sdf on a regular grid, in chunks."""
    mc, p, (sdf, dev, col, ren) = _tiny(R, seed=3)
    res = 20
    lo = torch.tensor([-1.0, -0.9, -0.8])
    hi = torch.tensor([1.0, 0.9, 1.1])
    u = ren.extract_fields(lo, hi, res, chunk=8)       # chunk does not divide the resolution
    assert u.shape == (res, res, res) and u.dtype == np.float32
    xs = [torch.linspace(float(lo[i]), float(hi[i]), res) for i in range(3)]
    xx, yy, zz = torch.meshgrid(*xs, indexing="ij")
    pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], dim=-1)
    ref = -O.sdf_forward(p, mc.sdf, pts)[:, 0].reshape(res, res, res)
    torch.testing.assert_close(torch.from_numpy(u), ref, rtol=1e-4, atol=2e-5)


def test_extract_fields_matches_the_reference_volume(R):
    """The same volume from the reference's own `extract_fields` (tests/golden/grid_tiny.npz, resolution 70 > its block
    size 64): `rnb_sdf_grid` (grid points generated in the kernel) within the point-wise SDF tolerance, and the native
    marching cubes of both volumes agree in vertex count to within the handful of cells a 1e-6 difference can flip."""
    import os
    from tests.golden_util import GOLDEN_DIR
    from oracle import mc_oracle as M
    z = np.load(os.path.join(GOLDEN_DIR, "grid_tiny.npz"), allow_pickle=False)
    s_, sf, c, r, rf = z["conf.sdf"], z["conf.sdf_f"], z["conf.color"], z["conf.render"], z["conf.render_f"]
    mc = O.ModelConf(
        sdf=O.SDFConf(d_in=int(s_[0]), d_out=int(s_[1]), d_hidden=int(s_[2]), n_layers=int(s_[3]),
                      skip_in=(int(s_[4]),) if s_[4] >= 0 else (), multires=int(s_[5]), bias=float(sf[0]), scale=float(sf[1])),
        color=O.ColorConf(d_feature=int(c[0]), d_in=int(c[1]), d_out=int(c[2]), d_hidden=int(c[3]), n_layers=int(c[4]),
                          multires_view=int(c[5])),
        render=O.RenderConf(n_samples=int(r[0]), n_importance=int(r[1]), n_outside=int(r[2]), up_sample_steps=int(r[3]),
                            perturb=float(rf[0])), init_val=float(rf[1]))
    p = {k[2:]: torch.from_numpy(z[k]).clone() for k in z.files if k.startswith("w.")}
    sdf, dev, col, ren = R.build_from_named_params(mc, p, device())
    res = int(z["resolution"])
    u = ren.extract_fields(torch.from_numpy(z["bound_min"]), torch.from_numpy(z["bound_max"]), res)
    ref = z["u"]
    assert u.shape == ref.shape == (res, res, res)
    np.testing.assert_allclose(u, ref, rtol=1e-4, atol=2e-5)
    v_dev, t_dev = R.marching_cubes(torch.from_numpy(u).to(device()), 0.0)
    v_ref, t_ref = M.marching_cubes(ref, 0.0)
    assert abs(len(v_dev) - len(v_ref)) <= max(4, len(v_ref) // 500) and len(v_ref) > 1000


def test_empty_batch_is_rejected_cleanly(R):
    mc, p, (sdf, dev, col, ren) = _tiny(R)
    e = torch.zeros(0, 3, device=device())
    with pytest.raises((RuntimeError, ValueError, R.native.NativeError)):
        ren.render_rnb(e, e, e[:, :1], e[:, :1], torch.zeros(3, 0, 1, 3, device=device()), cos_anneal_ratio=1.0)
    # the renderer is still usable afterwards
    batch = O.synthetic_batch(4, seed=1, step=0)
    b = {k: v.to(device()) for k, v in batch.items()}
    out = ren.render_rnb(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=1.0,
                         t_rand=b["t_rand"])
    assert bool(torch.isfinite(out["color_fine"]).all())


def test_large_batch_gradients_are_additive_over_shards(R):
    """Full-size networks, 4096 rays x 128 samples (8x the bench shape, 27 GB of saved state): with a loss that
    is a plain sum over rays, the parameter gradients of the whole batch equal the sum over two ragged shards
    rendered on the same depths — exercises every kernel's grid / split / offset arithmetic at size."""
    mc = O.ModelConf()
    torch.manual_seed(4)
    p = O.init_params(mc)
    with torch.no_grad():
        p["dev.variance"].fill_(0.35)
    sdf, dev, col, ren = R.build_from_named_params(mc, p, device())
    leaves = list(sdf.parameters()) + list(dev.parameters()) + list(col.parameters())
    batch = O.synthetic_batch(4096, seed=17, step=2)
    b = {k: v.to(device()) for k, v in batch.items()}

    def grads(lo, hi, z):
        for x in leaves:
            x.grad = None
        out = ren.render_rnb(b["rays_o"][lo:hi], b["rays_d"][lo:hi], b["near"][lo:hi], b["far"][lo:hi],
                             b["lights_dir"][:, lo:hi], cos_anneal_ratio=1.0, t_rand=b["t_rand"][lo:hi],
                             z_vals=None if z is None else z[lo:hi])
        zz = ren.last_z_vals
        (out["color_fine"].sum() + out["weight_sum"].sum() + (out["weights"] * out["cdf_fine"]).sum()).backward()
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(x.grad).all()) for x in leaves)
        return zz, [x.grad.detach().double().clone() for x in leaves]

    z, g_all = grads(0, 4096, None)
    _, g_a = grads(0, 1500, z)
    _, g_b = grads(1500, 4096, z)
    for x, ga, gb, name in zip(g_all, g_a, g_b, [n for n, _ in sdf.named_parameters()] + ["variance"]
                               + [n for n, _ in col.named_parameters()]):
        ref = ga + gb
        assert float((x - ref).norm()) <= 2e-4 * float(ref.norm()) + 1e-6, name


@pytest.mark.parametrize("warmup", [True, False])
def test_validate_image_call_shape_one_light_ragged_chunks(R, warmup):
    """`validate_image` (exp_runner.py:389-516) renders one view with ONE light, in chunks of `batch_size` rays: warm-up
    `render_rnb_warmup(..., lights_dir [1,1,1,3])` (:431-433), afterwards `render_rnb(..., lights_dir [1,b,1,3])` (:448), then
    builds the normal image `sum_s gradients * weights * inside_sphere` (:463-470).  Here: 37 rays in chunks of 16 / 16 / 5
    under no_grad (the forward-only path of the library), against the oracle on the depths the device sampled."""
    mc, p, (sdf, dev, col, ren) = _tiny(R, seed=5)
    B, chunk = 37, 16
    batch = O.synthetic_batch(B, seed=21, step=2, warmup=warmup)
    g = torch.Generator().manual_seed(9)
    one = torch.randn(1, 1, 1, 3, generator=g)
    one = one / one.norm()
    per_ray = torch.randn(1, B, 1, 3, generator=g)
    per_ray = per_ray / per_ray.norm(dim=-1, keepdim=True)
    colors, normals, n_chunks = [], [], 0
    with torch.no_grad():
        for lo in range(0, B, chunk):
            hi = min(B, lo + chunk)
            b = {k: batch[k][lo:hi].to(device()) for k in ("rays_o", "rays_d", "near", "far", "t_rand")}
            lights = one if warmup else per_ray[:, lo:hi]
            fn = ren.render_rnb_warmup if warmup else ren.render_rnb
            out = fn(b["rays_o"], b["rays_d"], b["near"], b["far"], lights.to(device()), cos_anneal_ratio=1.0,
                     t_rand=b["t_rand"])
            assert out["color_fine"].shape == (1, hi - lo, 3)
            assert out["gradients"].shape == (hi - lo, 32, 3) and out["inside_sphere"].shape == (hi - lo, 32)
            assert out["color_fine"].grad_fn is None
            z = ren.last_z_vals.cpu()
            ref = O.render_rnb(p, mc, batch["rays_o"][lo:hi], batch["rays_d"][lo:hi], batch["near"][lo:hi],
                               batch["far"][lo:hi], lights, cos_anneal_ratio=1.0, warmup=warmup, z_vals=z)
            for k in ("color_fine", "weights", "gradients", "inside_sphere", "weight_sum", "cdf_fine"):
                torch.testing.assert_close(out[k].cpu(), ref[k].detach(), rtol=1e-4, atol=2e-5, msg=lambda m: f"{k}: {m}")
            # the normal image of validate_image (exp_runner.py:463-470)
            n_img = (out["gradients"] * out["weights"][:, :32, None] * out["inside_sphere"][..., None]).sum(dim=1).cpu()
            n_ref = (ref["gradients"] * ref["weights"][:, :32, None] * ref["inside_sphere"][..., None]).sum(dim=1).detach()
            torch.testing.assert_close(n_img, n_ref, rtol=1e-4, atol=2e-5)
            colors.append(out["color_fine"].cpu())
            normals.append(n_img)
            n_chunks += 1
    assert n_chunks == 3 and torch.cat(colors, dim=1).shape == (1, B, 3) and torch.cat(normals).shape == (B, 3)
    assert float(torch.cat(normals).abs().max()) > 1e-3      # a surface was hit: the image is not empty
