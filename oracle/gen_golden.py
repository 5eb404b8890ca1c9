"""Golden-vector generator: runs the REFERENCE implementation and records plain arrays.

TEST INFRASTRUCTURE ONLY; runs only in the build container (needs /root/reference,
which does not exist on the GPU box).  It imports the reference's own
`models/{embedder,fields,renderer}.py` by path (two inert placeholder modules stand in
for `mcubes` / `icecream`, which are imported at renderer.py:6-7 but never used on the
path), drives `render`, `render_rnb`, `render_rnb_warmup` plus the train_rnb loss
(exp_runner.py:241-256, re-typed in oracle/rnb_oracle.py::rnb_loss because exp_runner.py
is not importable here) and writes inputs, intermediates, outputs and parameter gradients
as `.npz` files under tests/golden/.  No reference source or pickled object is stored.

    python oracle/gen_golden.py            # regenerates every fixture
"""
from __future__ import annotations

import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("RNB_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

from oracle import rnb_oracle as O  # noqa: E402


def import_reference():
    for name in ("mcubes", "icecream"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            if name == "icecream":
                m.ic = lambda *a, **k: None
            sys.modules[name] = m
    if REF not in sys.path:
        sys.path.insert(0, REF)
    warnings.filterwarnings("ignore", category=FutureWarning)
    from models.fields import SDFNetwork, RenderingNetwork, SingleVarianceNetwork  # type: ignore
    from models.renderer import NeuSRenderer  # type: ignore
    return SDFNetwork, RenderingNetwork, SingleVarianceNetwork, NeuSRenderer


def build_reference(mc: O.ModelConf, seed: int):
    SDFNetwork, RenderingNetwork, SingleVarianceNetwork, NeuSRenderer = import_reference()
    torch.manual_seed(seed)
    s, c, r = mc.sdf, mc.color, mc.render
    sdf = SDFNetwork(d_in=s.d_in, d_out=s.d_out, d_hidden=s.d_hidden, n_layers=s.n_layers,
                     skip_in=list(s.skip_in), multires=s.multires, bias=s.bias, scale=s.scale,
                     geometric_init=s.geometric_init, weight_norm=s.weight_norm)
    dev = SingleVarianceNetwork(mc.init_val)
    col = RenderingNetwork(d_feature=c.d_feature, mode=c.mode, d_in=c.d_in, d_out=c.d_out,
                           d_hidden=c.d_hidden, n_layers=c.n_layers, weight_norm=c.weight_norm,
                           multires_view=c.multires_view, squeeze_out=c.squeeze_out)
    ren = NeuSRenderer(None, sdf, dev, col, n_samples=r.n_samples, n_importance=r.n_importance,
                       n_outside=r.n_outside, up_sample_steps=r.up_sample_steps, perturb=r.perturb)
    ren.color_depth = c.d_out  # exp_runner.py:125
    return sdf, dev, col, ren


def named_params(sdf, dev, col):
    p = {}
    for k, v in sdf.named_parameters():
        p["sdf." + k] = v
    p["dev.variance"] = dev.variance
    for k, v in col.named_parameters():
        p["color." + k] = v
    return p


class Tracer:
    """Records the integer/intermediate tensors of the up-sampling loop of the reference."""

    def __init__(self, ren):
        self.ren = ren
        self.steps = []
        self.t_rand = None
        self._orig = {}

    def __enter__(self):
        ren = self.ren
        o_up, o_cat = ren.up_sample, ren.cat_z_vals
        o_ss, o_sort, o_rand = torch.searchsorted, torch.sort, torch.rand
        self._orig = dict(ss=o_ss, sort=o_sort, rand=o_rand)
        cur = {}

        def up(rays_o, rays_d, z_vals, sdf, n_importance, inv_s):
            cur.clear()
            cur["z_in"] = z_vals.detach().clone()
            cur["sdf_in"] = sdf.detach().clone()
            cur["inv_s"] = float(inv_s)
            out = o_up(rays_o, rays_d, z_vals, sdf, n_importance, inv_s)
            cur["new_z"] = out.detach().clone()
            return out

        def cat(rays_o, rays_d, z_vals, new_z_vals, sdf, last=False):
            z, s = o_cat(rays_o, rays_d, z_vals, new_z_vals, sdf, last=last)
            cur["z_out"] = z.detach().clone()
            cur["sdf_out"] = s.detach().clone()
            self.steps.append(dict(cur))
            return z, s

        def ss(*a, **k):
            r = o_ss(*a, **k)
            cur["inds"] = r.detach().clone()
            return r

        def sort(*a, **k):
            r = o_sort(*a, **k)
            cur["sort_index"] = r[1].detach().clone()
            return r

        def rand(*a, **k):
            if self.t_rand is not None:
                shape = a[0] if len(a) == 1 else a
                assert list(shape) == list(self.t_rand.shape), (shape, self.t_rand.shape)
                return self.t_rand.clone()
            return o_rand(*a, **k)

        o_core, o_mvps = ren.render_core, ren.render_core_mvps

        def core(rays_o, rays_d, z_vals, *a, **k):
            self.z_fine = z_vals.detach().clone()
            return o_core(rays_o, rays_d, z_vals, *a, **k)

        def mvps(rays_o, rays_d, z_vals, *a, **k):
            self.z_fine = z_vals.detach().clone()
            return o_mvps(rays_o, rays_d, z_vals, *a, **k)

        ren.up_sample, ren.cat_z_vals = up, cat
        ren.render_core, ren.render_core_mvps = core, mvps
        torch.searchsorted, torch.sort, torch.rand = ss, sort, rand
        return self

    def __exit__(self, *exc):
        torch.searchsorted = self._orig["ss"]
        torch.sort = self._orig["sort"]
        torch.rand = self._orig["rand"]
        del self.ren.up_sample
        del self.ren.cat_z_vals
        del self.ren.render_core
        del self.ren.render_core_mvps


class Replay:
    """Makes the reference's up-sampling loop return the sample positions recorded from an fp32 run (cast to the
    precision of the replaying modules), so that a second run of the reference in fp64 evaluates exactly the same
    samples: what follows the loop (render_core / render_core_mvps and the wrappers' composite) is then the
    reference's own code in fp64 on identical z_vals."""

    def __init__(self, ren, steps, t_rand, dtype, z_fine):
        self.ren, self.steps, self.t_rand, self.dtype, self.z_fine = ren, steps, t_rand, dtype, z_fine
        self.i = 0

    def __enter__(self):
        self._rand = torch.rand

        def up(rays_o, rays_d, z_vals, sdf, n_importance, inv_s):
            return self.steps[self.i]["new_z"].to(self.dtype)

        def cat(rays_o, rays_d, z_vals, new_z_vals, sdf, last=False):
            st = self.steps[self.i]
            self.i += 1
            return st["z_out"].to(self.dtype), st["sdf_out"].to(self.dtype)

        def rand(*a, **k):
            return self.t_rand.clone().to(self.dtype)

        o_core, o_mvps = self.ren.render_core, self.ren.render_core_mvps

        def core(rays_o, rays_d, z_vals, *a, **k):     # the fine pass sees exactly the fp32 run's z_vals
            return o_core(rays_o, rays_d, self.z_fine.to(self.dtype), *a, **k)

        def mvps(rays_o, rays_d, z_vals, *a, **k):
            return o_mvps(rays_o, rays_d, self.z_fine.to(self.dtype), *a, **k)

        self.ren.up_sample, self.ren.cat_z_vals = up, cat
        self.ren.render_core, self.ren.render_core_mvps = core, mvps
        torch.rand = rand
        return self

    def __exit__(self, *exc):
        torch.rand = self._rand
        del self.ren.up_sample
        del self.ren.cat_z_vals
        del self.ren.render_core
        del self.ren.render_core_mvps


def reference_fp64(mc, sdf, dev, col, ren, batch, tr_steps, z_fine, *, api, cos_anneal_ratio, no_albedo, perturb_overwrite,
                   background_rgb, with_grads):
    """The reference itself in double precision on the fp32 run's sample positions.  Returns (outputs, grads)."""
    rng = torch.get_rng_state()
    sdf64, dev64, col64, ren64 = build_reference(mc, seed=0)     # fresh modules (weight-normed ones do not deepcopy)
    torch.set_rng_state(rng)
    sdf64.load_state_dict(sdf.state_dict())
    dev64.load_state_dict(dev.state_dict())
    col64.load_state_dict(col.state_dict())
    sdf64, dev64, col64 = sdf64.double(), dev64.double(), col64.double()
    b = {k: v.double() for k, v in batch.items()}
    bg = background_rgb.double() if background_rgb is not None else None
    p64 = named_params(sdf64, dev64, col64)
    old_default = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)   # the reference creates helper tensors (linspace, ones) in the default dtype
    try:
        with Replay(ren64, tr_steps, batch["t_rand"], torch.float64, z_fine):
            if api == "render":
                out = ren64.render(b["rays_o"], b["rays_d"], b["near"], b["far"], perturb_overwrite=perturb_overwrite,
                                   background_rgb=bg, cos_anneal_ratio=cos_anneal_ratio)
            else:
                fn = ren64.render_rnb_warmup if api == "render_rnb_warmup" else ren64.render_rnb
                out = fn(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"],
                         perturb_overwrite=perturb_overwrite, background_rgb=bg, cos_anneal_ratio=cos_anneal_ratio,
                         no_albedo=no_albedo)
        grads = {}
        if with_grads:
            if api == "render":
                loss = (out["color_fine"] - b["true_rgb"][0]).abs().mean() + 0.1 * out["gradient_error"] \
                    + 0.1 * torch.nn.functional.binary_cross_entropy(
                        out["weight_sum"].clip(1e-3, 1 - 1e-3), (b["mask"] > 0.5).double())
            else:
                loss, _ = O.rnb_loss(out, b["true_rgb"], b["mask"])
            loss.backward()
            out = dict(out)
            out["loss"] = loss
            grads = {k: v.grad.detach() for k, v in p64.items() if v.grad is not None}
    finally:
        torch.set_default_dtype(old_default)
    return {k: v.detach() for k, v in out.items()}, grads


def conf_arrays(mc: O.ModelConf):
    s, c, r = mc.sdf, mc.color, mc.render
    return {
        "conf.sdf": np.array([s.d_in, s.d_out, s.d_hidden, s.n_layers, s.skip_in[0] if s.skip_in else -1,
                              s.multires], dtype=np.int64),
        "conf.sdf_f": np.array([s.bias, s.scale], dtype=np.float64),
        "conf.color": np.array([c.d_feature, c.d_in, c.d_out, c.d_hidden, c.n_layers, c.multires_view],
                               dtype=np.int64),
        "conf.render": np.array([r.n_samples, r.n_importance, r.n_outside, r.up_sample_steps],
                                dtype=np.int64),
        "conf.render_f": np.array([r.perturb, mc.init_val], dtype=np.float64),
    }


def run_case(name, mc, sdf, dev, col, ren, batch, *, api, cos_anneal_ratio, no_albedo=False,
             perturb_overwrite=-1, background_rgb=None, store_weights=True, grad_stride=1,
             with_grads=True, weights_from=None, grad64_stride=None):
    p = named_params(sdf, dev, col)
    for v in p.values():
        v.grad = None
    arrs = dict(conf_arrays(mc))
    arrs["meta.api"] = np.array(api)
    arrs["meta.cos_anneal_ratio"] = np.array(cos_anneal_ratio, dtype=np.float64)
    arrs["meta.no_albedo"] = np.array(int(no_albedo))
    arrs["meta.perturb_overwrite"] = np.array(perturb_overwrite, dtype=np.float64)
    arrs["meta.grad_stride"] = np.array(grad_stride)
    for k, v in batch.items():
        arrs["in." + k] = v.numpy()
    if background_rgb is not None:
        arrs["in.background_rgb"] = background_rgb.numpy()

    with Tracer(ren) as tr:
        tr.t_rand = batch["t_rand"]
        if api == "render":
            out = ren.render(batch["rays_o"], batch["rays_d"], batch["near"], batch["far"],
                             perturb_overwrite=perturb_overwrite, background_rgb=background_rgb,
                             cos_anneal_ratio=cos_anneal_ratio)
        else:
            fn = ren.render_rnb_warmup if api == "render_rnb_warmup" else ren.render_rnb
            out = fn(batch["rays_o"], batch["rays_d"], batch["near"], batch["far"], batch["lights_dir"],
                     perturb_overwrite=perturb_overwrite, background_rgb=background_rgb,
                     cos_anneal_ratio=cos_anneal_ratio, no_albedo=no_albedo)
    for i, st in enumerate(tr.steps):
        for k, v in st.items():
            arrs[f"trace.{i}.{k}"] = np.asarray(v.numpy() if torch.is_tensor(v) else v)
    arrs["trace.n_steps"] = np.array(len(tr.steps))
    arrs["trace.z_vals"] = tr.z_fine.numpy()     # what the fine pass (render_core / render_core_mvps) received
    for k, v in out.items():
        arrs["out." + k] = v.detach().numpy()

    if with_grads:
        if api == "render":
            # forward-only API in the reference (render_novel_image); loss on colour + eikonal
            tgt = batch["true_rgb"][0]
            loss = (out["color_fine"] - tgt).abs().mean() + 0.1 * out["gradient_error"] \
                + 0.1 * torch.nn.functional.binary_cross_entropy(
                    out["weight_sum"].clip(1e-3, 1 - 1e-3), (batch["mask"] > 0.5).float())
        else:
            loss, _ = O.rnb_loss(out, batch["true_rgb"], batch["mask"])
        loss.backward()
        arrs["out.loss"] = loss.detach().numpy()
        for k, v in p.items():
            if v.grad is None:
                continue
            g = v.grad.detach().reshape(-1)
            arrs["grad." + k] = g[::grad_stride].numpy().copy()
            arrs["gradnorm." + k] = np.array(float(g.double().norm()))
    # ---- the reference in fp64 on the same samples: calibrates the fp32 tolerances of the GPU tests --------
    out64, g64 = reference_fp64(mc, sdf, dev, col, ren, batch, tr.steps, tr.z_fine, api=api, cos_anneal_ratio=cos_anneal_ratio,
                                no_albedo=no_albedo, perturb_overwrite=perturb_overwrite,
                                background_rgb=background_rgb, with_grads=with_grads)
    for k, v in out64.items():
        if k in ("inside_sphere",):
            continue
        arrs["out64." + k] = v.numpy().astype(np.float64)
    # fp64 gradients: every element of the small tensors, every 16th (or grad_stride-th) of the large ones; rel32s is
    # the fp32 reference's own relative L2 distance from fp64 on exactly that subsample (rel32: whole tensor) — the
    # conditioning of the tensor, against which the GPU tests bound the HIP path's distance from fp64
    for k, g in g64.items():
        g = g.reshape(-1)
        g64s = 1 if g.numel() <= 4096 else (grad64_stride if grad64_stride is not None else max(grad_stride, 16))
        g32 = p[k].grad.detach().reshape(-1).double()
        arrs["grad64." + k] = g[::g64s].numpy().copy()
        arrs["grad64_stride." + k] = np.array(g64s)
        arrs["rel32." + k] = np.array(float((g32 - g).norm() / g.norm().clamp_min(1e-300)))
        arrs["rel32s." + k] = np.array(float((g32[::g64s] - g[::g64s]).norm() / g[::g64s].norm().clamp_min(1e-300)))
    if weights_from is not None:
        arrs["meta.weights_from"] = np.array(weights_from)
    elif store_weights:
        for k, v in p.items():
            arrs["w." + k] = v.detach().numpy().copy()
    else:
        for k, v in p.items():
            d = v.detach().double().reshape(-1)
            arrs["wsum." + k] = np.array([float(d.sum()), float((d * d).sum()), float(d[0]), float(d[-1])])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote {path}  ({os.path.getsize(path) / 1e6:.2f} MB)  loss={float(arrs.get('out.loss', np.nan)):.6f}")
    return out


def tiny_conf():
    return O.ModelConf(
        sdf=O.SDFConf(d_out=65, d_hidden=64, n_layers=8, skip_in=(4,), multires=6),
        color=O.ColorConf(d_feature=64, d_hidden=64, n_layers=2, multires_view=4),
        render=O.RenderConf(n_samples=16, n_importance=16, up_sample_steps=4, perturb=1.0),
        init_val=0.3)


def sharpen(mc, sdf, dev, col, ren, steps, B, lr=1e-3):
    """A few Adam steps of the reference's own train_rnb-shaped step so that no weight block
    stays at its zero/structured initial value; then a high inv_s (variance 0.6 => ~403)."""
    params = list(sdf.parameters()) + list(dev.parameters()) + list(col.parameters())
    opt = torch.optim.Adam(params, lr=lr)
    for it in range(steps):
        b = O.synthetic_batch(B, seed=7, step=it, warmup=(it % 2 == 0))
        torch.manual_seed(it)
        fn = ren.render_rnb_warmup if it % 2 == 0 else ren.render_rnb
        out = fn(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=1.0)
        loss, _ = O.rnb_loss(out, b["true_rgb"], b["mask"])
        opt.zero_grad()
        loss.backward()
        opt.step()
    with torch.no_grad():
        dev.variance.fill_(0.6)


def raygen_case():
    """Golden vectors of the reference's per-step ray generation (models/dataset.py:351-376) on a synthetic
    3-view / 3-light / 20x24 capture.  The Dataset class is instantiated without its file-reading __init__
    (needs OpenCV + image files); `cv2` is an inert placeholder module and `.cuda()` is the identity while the
    reference method runs (there is no GPU in the build container)."""
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")
    import_reference()
    from models.dataset import Dataset  # type: ignore
    g = torch.Generator().manual_seed(123)
    V, L, H, W = 3, 3, 20, 24
    ds = Dataset.__new__(Dataset)
    ds.H, ds.W, ds.n_images, ds.n_lights = H, W, V, L
    ds.images = torch.rand(V, L, H, W, 3, generator=g)
    ds.images_warmup = torch.rand(V, L, H, W, 3, generator=g)
    ds.masks = (torch.rand(V, H, W, generator=g) > 0.4).float().unsqueeze(3)
    ld = torch.randn(V, L, H, W, 3, generator=g)
    ds.light_directions = ld / ld.norm(dim=-1, keepdim=True)
    lw = torch.randn(V, L, 3, generator=g)
    ds.light_directions_warmup = lw / lw.norm(dim=-1, keepdim=True)
    K = torch.eye(4).repeat(V, 1, 1)
    K[:, 0, 0] = 30.0 + torch.rand(V, generator=g)
    K[:, 1, 1] = 31.0 + torch.rand(V, generator=g)
    K[:, 0, 2] = W / 2.0
    K[:, 1, 2] = H / 2.0
    ds.intrinsics_all_inv = torch.inverse(K)
    q, _ = torch.linalg.qr(torch.randn(V, 3, 3, generator=g))
    pose = torch.eye(4).repeat(V, 1, 1)
    pose[:, :3, :3] = q
    pose[:, :3, 3] = 3.0 * torch.nn.functional.normalize(torch.randn(V, 3, generator=g), dim=-1)
    ds.pose_all = pose
    out = {"images": ds.images, "images_warmup": ds.images_warmup, "masks": ds.masks,
           "light_directions": ds.light_directions, "light_directions_warmup": ds.light_directions_warmup,
           "intrinsics_all_inv": ds.intrinsics_all_inv, "pose_all": ds.pose_all}
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for case, (img_idx, B, seed) in enumerate([(0, 50, 7), (2, 2, 8), (1, 333, 9)]):   # B = 1 breaks the reference (.squeeze(), dataset.py:367)
            torch.random.manual_seed(seed)   # exp_runner.py:170 seeds before every draw
            data, wu, rgb, px, py = ds.ps_gen_random_rays_at_view_on_all_lights(img_idx, B)
            near, far = ds.near_far_from_sphere(data[:, :3], data[:, 3:6])
            lights = ds.light_directions[img_idx, :, py.cpu(), px.cpu(), :]     # exp_runner.py:214-218
            pre = f"c{case}_"
            out.update({pre + "img_idx": torch.tensor(img_idx), pre + "data": data, pre + "images_warmup": wu,
                        pre + "images": rgb, pre + "pixels_x": px, pre + "pixels_y": py, pre + "near": near,
                        pre + "far": far, pre + "lights_dir": lights})
    finally:
        torch.Tensor.cuda = orig_cuda
    path = os.path.join(OUT, "raygen_small.npz")
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


def train_step_reference(ren, opt, b, warmup, no_albedo=False):
    """One train_rnb iteration of the reference (exp_runner.py:174-263) on a prepared batch."""
    fn = ren.render_rnb_warmup if warmup else ren.render_rnb
    with Tracer(ren) as tr:       # only to feed the batch's t_rand through torch.rand
        tr.t_rand = b["t_rand"]
        out = fn(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=1.0,
                 no_albedo=no_albedo)
    loss, parts = O.rnb_loss(out, b["true_rgb"], b["mask"])
    opt.zero_grad()
    loss.backward()
    opt.step()
    return float(loss), out


def checkpoint_case():
    """A checkpoint in the reference's own layout (exp_runner.py:373-386): tiny networks + the reference's NeRF
    container, torch.optim.Adam over `nerf + sdf + variance + color` (exp_runner.py:105-115) after two train steps,
    written with torch.save as plain tensors / numbers (loads with weights_only=True).  The companion .npz holds the
    batch of step 3 and every parameter after the reference's step 3, so a test can load the checkpoint, take one
    step and compare."""
    import_reference()
    from models.fields import NeRF  # type: ignore
    mc = tiny_conf()
    sdf, dev, col, ren = build_reference(mc, seed=5)
    torch.manual_seed(6)
    nerf = NeRF(D=2, W=16, d_in=4, d_in_view=3, multires=2, multires_view=2, output_ch=4, skips=[1], use_viewdirs=True)
    params = list(nerf.parameters()) + list(sdf.parameters()) + list(dev.parameters()) + list(col.parameters())
    opt = torch.optim.Adam(params, lr=5e-4)
    for it in range(2):
        b = O.synthetic_batch(8, seed=21, step=it, warmup=(it == 0))
        train_step_reference(ren, opt, b, warmup=(it == 0))
    ckpt = {"nerf": nerf.state_dict(), "sdf_network_fine": sdf.state_dict(),
            "variance_network_fine": dev.state_dict(), "color_network_fine": col.state_dict(),
            "optimizer": opt.state_dict(), "iter_step": 2}
    path = os.path.join(OUT, "ref_ckpt_tiny.pth")
    torch.save(ckpt, path)
    torch.load(path, weights_only=True)   # must be loadable without executing anything
    b = O.synthetic_batch(8, seed=21, step=2, warmup=False)
    for g in opt.param_groups:
        g["lr"] = 3e-4                  # the schedule changes lr every step (exp_runner.py:327-337)
    loss, _ = train_step_reference(ren, opt, b, warmup=False)
    arrs = dict(conf_arrays(mc))
    for k, v in b.items():
        arrs["in." + k] = v.numpy()
    arrs["nerf.conf"] = np.array([2, 16, 4, 3, 2, 2, 4, 1], dtype=np.int64)
    arrs["n_nerf_params"] = np.array(len(list(nerf.parameters())))
    arrs["loss3"] = np.array(loss)
    for k, v in named_params(sdf, dev, col).items():
        arrs["after3." + k] = v.detach().numpy().copy()
    sd = opt.state_dict()
    for i, st in sd["state"].items():
        arrs[f"opt3.{i}.exp_avg"] = st["exp_avg"].numpy().copy()
        arrs[f"opt3.{i}.exp_avg_sq"] = st["exp_avg_sq"].numpy().copy()
    np.savez_compressed(os.path.join(OUT, "ref_ckpt_tiny_step3.npz"), **arrs)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB; loss of step 3:", loss)


def load_fixture_state(name, sdf, dev, col):
    """Loads the network state stored in tests/golden/<name>.npz (`w.*` arrays) into reference modules."""
    z = np.load(os.path.join(OUT, name + ".npz"), allow_pickle=False)
    w = {k[2:]: torch.from_numpy(z[k]).clone() for k in z.files if k.startswith("w.")}
    sdf.load_state_dict({k[4:]: v for k, v in w.items() if k.startswith("sdf.")})
    col.load_state_dict({k[6:]: v for k, v in w.items() if k.startswith("color.")})
    dev.load_state_dict({"variance": w["dev.variance"]})


def b512_case():
    """BASELINE config 2 at its real shape: full-size networks, 512 rays x (64+64) samples, `render_rnb`, on the
    sharpened state of full_main_sharp (a model that HAS a surface: inv_s ~ 403, weight_sum ~ 0.4-0.7), the
    reference's fp32 run + its fp64 replay, strided gradients.  The state is read back from full_main_sharp.npz, so
    the fixture regenerates identically whether or not the cases before it ran in the same process."""
    mc = O.ModelConf()
    sdf, dev, col, ren = build_reference(mc, seed=0)
    load_fixture_state("full_main_sharp", sdf, dev, col)
    b = O.synthetic_batch(512, seed=16, step=5, warmup=False)
    out = run_case("full_main_b512", mc, sdf, dev, col, ren, b, api="render_rnb", cos_anneal_ratio=1.0,
                   weights_from="full_main_sharp", grad_stride=61, grad64_stride=61)
    ws = out["weight_sum"].detach()
    print(f"  full_main_b512: weight_sum mean {float(ws.mean()):.3f}, weights.max {float(out['weights'].max()):.3f}, "
          f"d loss / d variance {float(dev.variance.grad):.3e}")


def flags_case():
    """Full-size (256-wide) networks — the shapes the fused HIP kernels take — under the flags the other full-size fixtures
    leave at their defaults: `cos_anneal_ratio` in {0.3, 0.0, 0.5}, `perturb_overwrite = 0` and `render`
    WITHOUT a background colour.  Same sharpened state as full_main_sharp (read back from its .npz), B = 32."""
    mc = O.ModelConf()
    sdf, dev, col, ren = build_reference(mc, seed=0)
    load_fixture_state("full_main_sharp", sdf, dev, col)
    B = 32
    b = O.synthetic_batch(B, seed=17, step=6, warmup=False)
    run_case("full_main_cos03", mc, sdf, dev, col, ren, b, api="render_rnb", cos_anneal_ratio=0.3,
             weights_from="full_main_sharp", grad_stride=7)
    # (batch seeds 20 / 26: picked among seeds 18..29 as the first ones on which the scene has a surface (weight_sum mean
    # > 0.4) and the fp32 reference resolves d loss / d variance — on seed 18 that gradient is 5e-3 from the reference's own
    # fp64 run with cos_anneal_ratio = 0, which tests/golden_util.py refuses as a parity target)
    b = O.synthetic_batch(B, seed=20, step=9, warmup=True)
    run_case("full_warmup_cos0_noperturb", mc, sdf, dev, col, ren, b, api="render_rnb_warmup", cos_anneal_ratio=0.0,
             perturb_overwrite=0, weights_from="full_main_sharp", grad_stride=7)
    b = O.synthetic_batch(B, seed=26, step=15, warmup=False)
    run_case("full_render_nobg_cos05", mc, sdf, dev, col, ren, b, api="render", cos_anneal_ratio=0.5,
             weights_from="full_main_sharp", grad_stride=7)


def odd_case():
    """Odd sample counts: the tiny networks in the state of tiny_main_sharp (read back from its .npz) at 17 + 15 / 3 —
    torch.linspace over 17 depths (its two halves differ), three up-sampling steps of n_new = 5 on n = 17, 22, 27
    (linspace over 5 quantiles, searchsorted and sort at odd sizes), S = 32.  `render_rnb`, 8 rays.  Written on its own
    (`python oracle/gen_golden.py odd`): no other fixture is regenerated."""
    import dataclasses
    mc = tiny_conf()
    mc = dataclasses.replace(mc, render=dataclasses.replace(mc.render, n_samples=17, n_importance=15, up_sample_steps=3))
    sdf, dev, col, ren = build_reference(mc, seed=0)
    load_fixture_state("tiny_main_sharp", sdf, dev, col)
    b = O.synthetic_batch(8, seed=8, step=7, warmup=False)
    out = run_case("tiny_main_odd_17x15", mc, sdf, dev, col, ren, b, api="render_rnb", cos_anneal_ratio=0.3,
                   weights_from="tiny_main_sharp")
    print(f"  tiny_main_odd_17x15: weight_sum mean {float(out['weight_sum'].detach().mean()):.3f}")


def grid_case():
    """The SDF grid of validate_mesh from the REFERENCE's own `extract_fields` (models/renderer.py:10-25, called with
    query_func = -sdf_network.sdf as at :1219-1224): tiny networks (seed 0 state of tiny_warmup_geo), asymmetric bounds,
    resolution 70 — larger than the reference's block size N = 64, so its chunked evaluation is exercised."""
    import_reference()
    from models.renderer import extract_fields  # type: ignore
    mc = tiny_conf()
    sdf, dev, col, ren = build_reference(mc, seed=0)
    lo = torch.tensor([-1.0, -0.9, -0.8])
    hi = torch.tensor([1.0, 0.9, 1.1])
    res = 70
    u = extract_fields(lo, hi, res, lambda pts: -sdf.sdf(pts))
    arrs = dict(conf_arrays(mc))
    arrs["bound_min"], arrs["bound_max"], arrs["resolution"] = lo.numpy(), hi.numpy(), np.array(res)
    arrs["u"] = u.astype(np.float32)
    for k, v in named_params(sdf, dev, col).items():
        arrs["w." + k] = v.detach().numpy().copy()
    path = os.path.join(OUT, "grid_tiny.npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB): u in [{u.min():.3f}, {u.max():.3f}]")


CONV = dict(B=64, steps=200, warm_steps=100, lr=5e-4, warm_up_end=20, end_iter=200, alpha=0.05, eval_steps=4)


def convergence_run(threads):
    """One 200-step training run of the reference (see convergence_case) with the given number of CPU threads."""
    c = CONV
    torch.set_num_threads(threads)
    mc = O.ModelConf()
    sdf, dev, col, ren = build_reference(mc, seed=0)
    params = list(sdf.parameters()) + list(dev.parameters()) + list(col.parameters())
    opt = torch.optim.Adam(params, lr=c["lr"])
    losses = []
    import time
    t0 = time.time()
    for it in range(c["steps"]):
        for g in opt.param_groups:
            g["lr"] = c["lr"] * O.lr_factor(it, c["warm_up_end"], c["end_iter"], c["alpha"])
        warm = it < c["warm_steps"]
        b = O.sphere_scene_batch(c["B"], seed=31, step=it, warmup=warm)
        loss, _ = train_step_reference(ren, opt, b, warmup=warm)
        losses.append(loss)
        if it % 40 == 0:
            print(f"  conv[{threads} threads] it {it}: loss {loss:.5f}  ({time.time() - t0:.0f} s)", flush=True)
    # held-out evaluation: PSNR of the rendered colours inside the silhouette, main mode, no perturbation
    se, n, wsum_err = 0.0, 0, 0.0
    for k in range(c["eval_steps"]):
        b = O.sphere_scene_batch(c["B"], seed=31, step=1000 + k, warmup=False)
        with Tracer(ren) as tr:
            tr.t_rand = b["t_rand"]
            out = ren.render_rnb(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], perturb_overwrite=0,
                                 cos_anneal_ratio=1.0)
        m = b["mask"][None]
        se += float((((out["color_fine"].detach() - b["true_rgb"]) * m) ** 2).sum())
        n += int(m.sum()) * 3 * 3
        wsum_err += float((out["weight_sum"].detach() - b["mask"]).abs().mean())
    psnr = -10.0 * np.log10(se / n)
    return np.array(losses, dtype=np.float64), psnr, wsum_err / c["eval_steps"], named_params(sdf, dev, col)


def convergence_case():
    """BASELINE config 1 (64 rays x (64+64) samples, 200 iterations): the REFERENCE trained on the analytic sphere
    capture of oracle/rnb_oracle.py::sphere_scene_batch with the schedule of exp_runner.py:320-332 (scaled to 200
    iterations), first half render_rnb_warmup, second half render_rnb.  Stores the loss curve, the final PSNR on
    held-out batches and parameter checksums — TWICE: with 8 and with 3 CPU threads.  The two runs differ only in the
    summation order of the CPU GEMMs, and their trajectories already differ by up to 27 % per decile of the run (the
    up-sampling loop amplifies last-bit differences into different samples): the pair is the yardstick for how
    closely any other implementation can be expected to track "the" reference curve."""
    c = CONV
    losses, psnr, mask_l1, params = convergence_run(8)
    losses_alt, psnr_alt, mask_l1_alt, _ = convergence_run(3)
    torch.set_num_threads(8)
    arrs = {"losses": losses, "psnr": np.array(psnr), "mask_l1": np.array(mask_l1),
            "losses_alt": losses_alt, "psnr_alt": np.array(psnr_alt), "mask_l1_alt": np.array(mask_l1_alt),
            "conf": np.array([c["B"], c["steps"], c["warm_steps"], c["warm_up_end"], c["end_iter"], c["eval_steps"]]),
            "conf_f": np.array([c["lr"], c["alpha"]])}
    for k, v in params.items():
        d = v.detach().double().reshape(-1)
        arrs["wsum." + k] = np.array([float(d.sum()), float((d * d).sum())])
    np.savez_compressed(os.path.join(OUT, "convergence_ref.npz"), **arrs)
    da, db = losses.reshape(10, -1).mean(1), losses_alt.reshape(10, -1).mean(1)
    print(f"wrote convergence_ref.npz: loss {losses[0]:.4f} -> {losses[-1]:.4f}, PSNR {psnr:.2f} dB (3 threads: "
          f"{psnr_alt:.2f} dB), mask L1 {mask_l1:.4f} / {mask_l1_alt:.4f}; max decile deviation between the two "
          f"reference runs {float((np.abs(da - db) / da).max()):.3f}")


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)

    # ---- (i) tiny networks: every API / flag combination, full weights + full grads -------------
    mc = tiny_conf()
    sdf, dev, col, ren = build_reference(mc, seed=0)
    B = 8
    b = O.synthetic_batch(B, seed=1, step=0, warmup=True)
    run_case("tiny_warmup_geo", mc, sdf, dev, col, ren, b, api="render_rnb_warmup", cos_anneal_ratio=1.0)
    sharpen(mc, sdf, dev, col, ren, steps=60, B=16, lr=2e-3)
    b = O.synthetic_batch(B, seed=2, step=1, warmup=True)
    run_case("tiny_warmup_sharp", mc, sdf, dev, col, ren, b, api="render_rnb_warmup", cos_anneal_ratio=1.0)
    b = O.synthetic_batch(B, seed=3, step=2, warmup=False)
    run_case("tiny_main_sharp", mc, sdf, dev, col, ren, b, api="render_rnb", cos_anneal_ratio=0.3)
    b = O.synthetic_batch(B, seed=4, step=3, warmup=False)
    run_case("tiny_main_noalbedo", mc, sdf, dev, col, ren, b, api="render_rnb", cos_anneal_ratio=0.0,
             no_albedo=True)
    b = O.synthetic_batch(B, seed=5, step=4, warmup=False)
    run_case("tiny_render_bg", mc, sdf, dev, col, ren, b, api="render", cos_anneal_ratio=1.0,
             perturb_overwrite=0, background_rgb=torch.ones(1, 3))
    b = O.synthetic_batch(B, seed=6, step=5, warmup=False)
    run_case("tiny_render_nobg", mc, sdf, dev, col, ren, b, api="render", cos_anneal_ratio=0.5)

    # ---- (ii) full-size networks at the config-1 shape (B=64, 64+64) --------------------------
    mc = O.ModelConf()
    sdf, dev, col, ren = build_reference(mc, seed=0)
    B = 64
    b = O.synthetic_batch(B, seed=11, step=0, warmup=True)
    # geometric-init weights are reproducible from the seed: store checksums + strided grads
    run_case("full_warmup_geo", mc, sdf, dev, col, ren, b, api="render_rnb_warmup", cos_anneal_ratio=1.0,
             store_weights=False, grad_stride=7)
    sharpen(mc, sdf, dev, col, ren, steps=30, B=32, lr=1e-3)
    b = O.synthetic_batch(B, seed=12, step=1, warmup=False)
    run_case("full_main_sharp", mc, sdf, dev, col, ren, b, api="render_rnb", cos_anneal_ratio=1.0,
             store_weights=True, grad_stride=1)
    # the same sharpened full-size state (weights read from full_main_sharp.npz) through the other entry points:
    # R5 `render` (config "render_core" named by the north star), BASELINE config 3 (`no_albedo`: the feature rows of
    # lin8 and the albedo net get no gradient) and BASELINE config 1's n_importance = 0 shape (S = 64)
    B = 32
    b = O.synthetic_batch(B, seed=13, step=2, warmup=False)
    run_case("full_render_sharp", mc, sdf, dev, col, ren, b, api="render", cos_anneal_ratio=1.0,
             background_rgb=torch.ones(1, 3), weights_from="full_main_sharp", grad_stride=7)
    b = O.synthetic_batch(B, seed=14, step=3, warmup=False)
    run_case("full_main_noalbedo", mc, sdf, dev, col, ren, b, api="render_rnb", cos_anneal_ratio=1.0,
             no_albedo=True, weights_from="full_main_sharp", grad_stride=7)
    import dataclasses
    mc64 = dataclasses.replace(mc, render=dataclasses.replace(mc.render, n_importance=0))
    _, _, _, NeuSRenderer = import_reference()
    ren64s = NeuSRenderer(None, sdf, dev, col, n_samples=64, n_importance=0, n_outside=0, up_sample_steps=4, perturb=1.0)
    ren64s.color_depth = mc.color.d_out
    b = O.synthetic_batch(B, seed=15, step=4, warmup=True)
    run_case("full_warmup_s64", mc64, sdf, dev, col, ren64s, b, api="render_rnb_warmup", cos_anneal_ratio=1.0,
             weights_from="full_main_sharp", grad_stride=7)
    # ---- (iii) BASELINE config 2 at its real shape (B = 512) on the same sharpened state ---------
    b512_case()
    # ---- (iv) the non-default flags on the full-size networks ----------------------------------------
    flags_case()
    # ---- (v) odd sample counts on the tiny networks ---------------------------------------------------
    odd_case()


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] in ("raygen", "checkpoint", "convergence", "b512", "grid", "flags", "odd"):
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    {"raygen": raygen_case, "checkpoint": checkpoint_case, "convergence": convergence_case,
     "b512": b512_case, "grid": grid_case, "flags": flags_case, "odd": odd_case}[sys.argv[1]]()
    sys.exit(0)

if __name__ == "__main__":
    main()
    raygen_case()
    checkpoint_case()
    grid_case()
    convergence_case()
