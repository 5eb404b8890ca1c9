"""Cost of the render's input gradients: config 2 (512 rays x (64 + 64) samples, fp32 default variant), render_rnb +
rnb_loss + backward, with and without rays_o, rays_d and lights_dir requiring grad.  The two legs alternate step by step in
one process; each step is timed with device events (render start -> backward end); medians of --steps per leg.  Prints
one JSON line with the build id and the added time per step.

  python tools/render_input_grad_bench.py [--steps 60] [--warmup 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rnb_neus_fork_amd as R  # noqa: E402
from oracle import rnb_oracle as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rays", type=int, default=512)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    mc = O.ModelConf()   # 256-wide shipped shape, 64 + 64 samples
    torch.manual_seed(0)
    p = O.init_params(mc)
    sdf, devn, col, ren = R.build_from_named_params(mc, p, dev)
    batch = {k: v.to(dev) for k, v in O.synthetic_batch(a.rays, seed=3, step=1).items()}

    def step(inputs):
        x = {k: v.detach().requires_grad_(inputs and k in ("rays_o", "rays_d", "lights_dir")) for k, v in batch.items()}
        for net in (sdf, devn, col):
            for q in net.parameters():
                q.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = ren.render_rnb(x["rays_o"], x["rays_d"], x["near"], x["far"], x["lights_dir"], cos_anneal_ratio=1.0,
                             t_rand=x["t_rand"])
        R.rnb_loss(out, x["true_rgb"], x["mask"])[0].backward()
        e1.record()
        torch.cuda.synchronize()
        if inputs:
            assert all(x[k].grad is not None for k in ("rays_o", "rays_d", "lights_dir"))
        return e0.elapsed_time(e1)

    for i in range(2 * a.warmup):
        step(i % 2 == 1)
    t = {False: [], True: []}
    for i in range(2 * a.steps):
        leg = i % 2 == 1
        t[leg].append(step(leg))
    base, with_in = statistics.median(t[False]), statistics.median(t[True])
    print(json.dumps({"build_id": R.native.build_id(), "rays": a.rays, "samples": 128, "steps_per_leg": a.steps,
                      "ms_per_step_plain": round(base, 4), "ms_per_step_input_grads": round(with_in, 4),
                      "added_ms": round(with_in - base, 4), "target_added_ms": 0.15,
                      "plain_p10_p90": [round(sorted(t[False])[len(t[False]) // 10], 4),
                                        round(sorted(t[False])[len(t[False]) * 9 // 10], 4)],
                      "input_grads_p10_p90": [round(sorted(t[True])[len(t[True]) // 10], 4),
                                              round(sorted(t[True])[len(t[True]) * 9 // 10], 4)]}))


if __name__ == "__main__":
    main()
