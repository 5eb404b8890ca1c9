"""Cost of camera refinement in the config-2 step (512 rays x (64 + 64) samples, the shipped 256-wide networks, fp32
default variant): DeviceRays.sample -> render_rnb -> rnb_loss -> backward -> FlatAdam on a synthetic source-mode capture.

Legs, alternating step by step in one process, each step timed with device events from the start of `sample` to the end
of the optimizer steps; medians of --steps per leg:
  off     no refinement: today's step
  inputs  no refinement, but rays_o, rays_d and lights_dir are detached leaves that require grad: the step pays the
          render's input-gradient backward (profiles/render_input_grads.txt) and nothing else
  on      `set_refinement(CameraRefinement(V, refine_focal=True))` with a torch Adam of the caller's on its parameters
`on - inputs` is what refinement itself adds: the camera parametrisation (torch ops on 3-vectors, forward and backward),
`rnb_gen_rays_camera_bwd` and the small optimizer.  `--legs off` runs the one leg that another build of the package has
too; `--tree DIR` imports the package (and the oracle) from another checkout, so that the off leg can alternate with a
parent build process by process.  Prints one JSON line with the build id.

  python tools/camera_refine_bench.py [--steps 60] [--warmup 10] [--legs off,inputs,on] [--tree DIR]
  python tools/camera_refine_bench.py --recover        # pose recovery demonstration (logged, not a test)
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch


def _capture(R, dev, V, H, W, seed=0):
    """A synthetic source-mode capture: cameras on the radius-3 sphere looking at the origin with a field of view that just
    holds the unit sphere, random camera-facing u8 normals and u8 albedo, the silhouette of the radius-0.5 ball as mask."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(V, 3, generator=g)
    c = 3.0 * c / c.norm(dim=-1, keepdim=True)
    fwd = -c / c.norm(dim=-1, keepdim=True)
    up0 = torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd).clone()
    up0[fwd[:, 2].abs() > 0.9] = torch.tensor([1.0, 0.0, 0.0])
    right = torch.linalg.cross(up0, fwd)
    right = right / right.norm(dim=-1, keepdim=True)
    up = torch.linalg.cross(fwd, right)
    pose = torch.eye(4).repeat(V, 1, 1)
    pose[:, :3, 0], pose[:, :3, 1], pose[:, :3, 2], pose[:, :3, 3] = right, up, fwd, c
    K = torch.eye(4)
    K[0, 0] = K[1, 1] = 0.5 * min(H, W) / math.tan(math.asin(1.0 / 3.0))
    K[0, 2], K[1, 2] = W / 2.0, H / 2.0
    kinv = torch.inverse(K).repeat(V, 1, 1)
    normals = torch.randint(0, 256, (V, H, W, 3), generator=g, dtype=torch.uint8)
    normals[..., 2] = normals[..., 2] // 2 + 128          # decoded n_z = -(2c - 1) < 0: facing the camera
    albedo = torch.randint(0, 256, (V, H, W, 3), generator=g, dtype=torch.uint8)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], -1)
    masks = torch.empty(V, H, W, dtype=torch.uint8)
    for v in range(V):
        d = pix @ kinv[v, :3, :3].T
        d = (d / d.norm(dim=-1, keepdim=True)) @ pose[v, :3, :3].T
        closest = c[v] + d * (-(c[v] * d).sum(-1, keepdim=True))
        masks[v] = (closest.norm(dim=-1) < 0.5).to(torch.uint8) * 255
    return R.DeviceRays.from_source_maps(normals, albedo, masks, kinv, pose, dev), pose, kinv


def _model(R, O, dev):
    mc = O.ModelConf()   # 256-wide shipped shape, 64 + 64 samples
    torch.manual_seed(0)
    return R.build_from_named_params(mc, O.init_params(mc), dev)


def bench(R, O, a):
    dev = torch.device("cuda:0")
    legs = a.legs.split(",")
    sdf, devn, col, ren = _model(R, O, dev)
    params = [q for net in (sdf, devn, col) for q in net.parameters()]
    opt = R.FlatAdam(params, lr=5e-4)
    rays, _, _ = _capture(R, dev, a.views, a.size, a.size)
    refine = cam_opt = None
    if "on" in legs:
        refine = R.CameraRefinement(a.views, refine_focal=True).to(dev)
        cam_opt = torch.optim.Adam(refine.parameters(), lr=1e-4)

    def step(leg, i):
        v = i % a.views
        if leg == "on":
            rays.set_refinement(refine)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s = rays.sample(v, a.rays)
        o, d, lights = s["rays_o"], s["rays_d"], s["lights_dir"]
        if leg == "inputs":
            o, d, lights = (t.detach().requires_grad_(True) for t in (o, d, lights))
        out = ren.render_rnb(o, d, s["near"], s["far"], lights, cos_anneal_ratio=1.0)
        R.rnb_loss(out, s["true_rgb"], s["mask"])[0].backward()
        opt.step()
        opt.zero_grad()
        if leg == "on":
            cam_opt.step()
            cam_opt.zero_grad()
        e1.record()
        torch.cuda.synchronize()
        if leg == "on":
            rays.set_refinement(None)
        return e0.elapsed_time(e1)

    for i in range(a.warmup * len(legs)):
        step(legs[i % len(legs)], i)
    t = {leg: [] for leg in legs}
    for i in range(a.steps * len(legs)):
        leg = legs[i % len(legs)]
        t[leg].append(step(leg, i))
    line = {"build_id": R.native.build_id(), "tree": os.path.relpath(a.tree), "rays": a.rays, "samples": 128,
            "capture": f"{a.views}x{a.size}x{a.size} u8 source maps", "steps_per_leg": a.steps}
    for leg in legs:
        q = sorted(t[leg])
        line[f"ms_per_step_{leg}"] = round(statistics.median(q), 4)
        line[f"{leg}_p10_p90"] = [round(q[len(q) // 10], 4), round(q[len(q) * 9 // 10], 4)]
    if "on" in legs and "inputs" in legs and "off" in legs:
        line["input_grads_added_ms"] = round(line["ms_per_step_inputs"] - line["ms_per_step_off"], 4)
        line["refinement_added_ms"] = round(line["ms_per_step_on"] - line["ms_per_step_inputs"], 4)
    print(json.dumps(line))


def recover(R, O, a):
    """Networks frozen at the geometric init; targets rendered from the true camera; the stored pose of one view is off by
    0.02 along a fixed direction; Adam on that view's tau alone.  Logs |stored t + tau - true t| per step."""
    dev = torch.device("cuda:0")
    sdf, devn, col, ren = _model(R, O, dev)
    for net in (sdf, devn, col):
        for q in net.parameters():
            q.requires_grad_(False)
    true_rays, pose, kinv = _capture(R, dev, a.views, a.size, a.size)
    v = 1
    offset = 0.02 * torch.tensor([2.0, -1.0, 2.0]) / 3.0
    wrong = pose.clone()
    wrong[v, :3, 3] += offset
    rays = R.DeviceRays.from_source_maps(true_rays.normals, true_rays.albedos, true_rays.masks, kinv, wrong, dev)
    refine = R.CameraRefinement(a.views).to(dev)
    rays.set_refinement(refine)
    cam_opt = torch.optim.Adam([refine.pose_delta], lr=2e-3)
    gen = torch.Generator().manual_seed(1)
    log = []
    for i in range(a.recover_steps):
        px = torch.randint(0, a.size, (a.rays,), generator=gen)
        py = torch.randint(0, a.size, (a.rays,), generator=gen)
        with torch.no_grad():
            t = true_rays.sample(v, a.rays, pixels_x=px, pixels_y=py)
            want = ren.render_rnb(t["rays_o"], t["rays_d"], t["near"], t["far"], t["lights_dir"], cos_anneal_ratio=1.0,
                                  perturb_overwrite=0)
        s = rays.sample(v, a.rays, pixels_x=px, pixels_y=py)
        out = ren.render_rnb(s["rays_o"], s["rays_d"], s["near"], s["far"], s["lights_dir"], cos_anneal_ratio=1.0,
                             perturb_overwrite=0)
        loss = R.rnb_loss(out, want["color_fine"], (want["weight_sum"] > 0.5).float())[0]
        cam_opt.zero_grad()
        loss.backward()
        refine.pose_delta.grad[:, :3] = 0.0          # tau alone
        cam_opt.step()
        err = float((refine.pose_delta.detach()[v, 3:].cpu() + offset).norm())
        log.append((i, float(loss.detach()), err))
    for i, loss, err in log:
        if i % 5 == 0 or i + 1 == len(log):
            print(f"recover step {i:3d}: loss {loss:.6f}  |t + tau - t_true| {err:.5f}")
    print(json.dumps({"build_id": R.native.build_id(), "recover": True, "rays": a.rays, "steps": a.recover_steps,
                      "offset": round(float(offset.norm()), 5), "error_first": round(log[0][2], 5),
                      "error_last": round(log[-1][2], 5), "error_min": round(min(e for _, _, e in log), 5)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rays", type=int, default=512)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--legs", default="off,inputs,on")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--recover", action="store_true")
    ap.add_argument("--recover-steps", type=int, default=60)
    a = ap.parse_args()
    unknown = set(a.legs.split(",")) - {"off", "inputs", "on"}
    if unknown:
        ap.error(f"unknown legs {sorted(unknown)}")
    sys.path.insert(0, os.path.abspath(a.tree))
    import rnb_neus_fork_amd as R
    from oracle import rnb_oracle as O
    if not torch.cuda.is_available():
        raise SystemExit("camera_refine_bench: needs a GPU (there is no CPU path)")
    (recover if a.recover else bench)(R, O, a)


if __name__ == "__main__":
    main()
