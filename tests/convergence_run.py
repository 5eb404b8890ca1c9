"""The 200-step training run of the convergence test (tests/test_gpu_convergence.py, which documents the fixture and the
envelope) and the envelope's width: shared with tools/conv_spread.py.  Not a test module."""
import os

import numpy as np
import torch

from oracle import rnb_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

ENVELOPE = 0.15        # widening of the [min, max] band spanned by the two reference runs, per decile (measured: fp32
                       # 2.8 % and bf16 3.9 % INSIDE an un-widened... i.e. 10 %-widened band; the fp32 atomics of the weight
                       # gradients make a run differ from the next in the last bits, hence the margin)


def train(R, z, variant):
    dev = torch.device("cuda:0")
    B, steps, warm_steps, warm_up_end, end_iter, eval_steps = (int(v) for v in z["conf"])
    lr, alpha = (float(v) for v in z["conf_f"])
    torch.manual_seed(0)
    sdf = R.SDFNetwork(d_out=257, d_in=3, d_hidden=256, n_layers=8, skip_in=[4], multires=6, bias=0.5, scale=1.0,
                       geometric_init=True, weight_norm=True).to(dev)
    devn = R.SingleVarianceNetwork(0.3).to(dev)
    col = R.RenderingNetwork(d_feature=256, mode="no_view_dir", d_in=6, d_out=3, d_hidden=256, n_layers=2,
                             weight_norm=True, multires_view=4, squeeze_out=True).to(dev)
    ren = R.NeuSRenderer(None, sdf, devn, col, n_samples=64, n_importance=64, n_outside=0, up_sample_steps=4, perturb=1.0)
    ren.set_variant(**variant)
    opt = R.FlatAdam(list(sdf.parameters()) + list(devn.parameters()) + list(col.parameters()), lr=lr)
    losses = []
    for it in range(steps):
        opt.param_groups[0]["lr"] = lr * O.lr_factor(it, warm_up_end, end_iter, alpha)
        warm = it < warm_steps
        b = {k: v.to(dev) for k, v in O.sphere_scene_batch(B, seed=31, step=it, warmup=warm).items()}
        fn = ren.render_rnb_warmup if warm else ren.render_rnb
        out = fn(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=1.0,
                 t_rand=b["t_rand"])
        loss, _ = R.rnb_loss(out, b["true_rgb"], b["mask"])
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu().double().numpy()
    se, n, wsum_err = 0.0, 0, 0.0
    with torch.no_grad():
        for k in range(eval_steps):
            b = {kk: v.to(dev) for kk, v in O.sphere_scene_batch(B, seed=31, step=1000 + k, warmup=False).items()}
            out = ren.render_rnb(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], perturb_overwrite=0,
                                 cos_anneal_ratio=1.0)
            m = b["mask"][None]
            se += float((((out["color_fine"] - b["true_rgb"]) * m) ** 2).sum())
            n += int(m.sum()) * 9
            wsum_err += float((out["weight_sum"] - b["mask"]).abs().mean())
    return losses, -10.0 * np.log10(se / n), wsum_err / eval_steps
