"""Resident bytes and ray-generation time of the two modes of `DeviceRays` on one synthetic capture, in the same run:

  stack   `DeviceRays(images, images_warmup, masks, light_directions, ...)`: the finished float32 stacks of the reference's
          `Dataset.__init__`, gathered by rnb_gen_rays_at_view / rnb_gen_rays_grid
  source  `DeviceRays.from_source_maps(normals, albedos, masks, ...)`: 8-bit normal, albedo and mask maps; lights and colours
          computed per requested pixel by rnb_gen_rays_at_view_from_maps / rnb_gen_rays_grid_from_maps

The capture (default 20 views of 512 x 612, so that both modes fit comfortably) is generated on the device from a seed:
camera-facing unit normals quantised to 8 bits, random albedo, a disc mask; the stacks of stack mode are what source mode's
`materialize` gives for every view, so both modes hold the same capture.

Timed with device events around each call (the call's own launches: `sample` draws its pixels on the device, then one
kernel), after a warm-up, the two modes alternating call by call, views cycling.  Per mode: the median over all timed
calls, and the medians of `--rounds` consecutive blocks of calls; the spread of a mode is the largest minus the smallest
block median.  Acceptance line: source-mode `sample` may be slower than stack-mode `sample` by no more than stack mode's
own spread.  The whole-view `view_rays` figure is reported only.  Run it under a `timeout`:

  timeout 600 python tools/source_maps_raygen_bench.py --out profiles/source_maps_raygen.txt
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_source_maps(V, H, W, dev, seed=0):
    """uint8 normals / albedo [V,H,W,3] and masks [V,H,W] on the device, and look-at cameras on the radius-3 sphere"""
    g = torch.Generator(device=dev).manual_seed(seed)
    n = torch.randn(V, H, W, 3, device=dev, generator=g)
    n[..., 2] = -n[..., 2].abs() - 0.05                                   # camera-facing (the reference's convention)
    n = n / n.norm(dim=-1, keepdim=True)
    enc = n * torch.tensor([1.0, -1.0, -1.0], device=dev)                  # the inverse of load_normal
    normals = ((enc + 1.0) * 0.5 * 255.0).round().clamp(0, 255).to(torch.uint8)
    albedo = torch.randint(0, 256, (V, H, W, 3), device=dev, generator=g, dtype=torch.uint8)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    disc = ((xs - W / 2) ** 2 + (ys - H / 2) ** 2) < (0.4 * min(H, W)) ** 2
    masks = (disc.to(torch.uint8) * 255).expand(V, H, W).contiguous()
    gv = torch.Generator("cpu").manual_seed(seed)
    c = torch.randn(V, 3, generator=gv)
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
    K[0, 0] = K[1, 1] = 1.4 * min(H, W)
    K[0, 2], K[1, 2] = W / 2.0, H / 2.0
    return normals, albedo, masks, torch.inverse(K).repeat(V, 1, 1), pose


def timed(calls, n, warmup, rounds):
    """`calls`: name -> function of the call's number.  Returns name -> (all times in microseconds, block medians)."""
    names = list(calls)
    for i in range(warmup):
        for k in names:
            calls[k](i)
    torch.cuda.synchronize()
    events = {k: [] for k in names}
    for i in range(n):
        for k in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            calls[k](i)
            e1.record()
            events[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {}
    for k in names:
        t = [1e3 * a.elapsed_time(b) for a, b in events[k]]
        per = max(1, n // rounds)
        out[k] = (t, [statistics.median(t[j:j + per]) for j in range(0, per * rounds, per) if t[j:j + per]])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=612)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--launches", type=int, default=1000, help="timed sample() calls per mode")
    ap.add_argument("--view-launches", type=int, default=100, help="timed whole-view view_rays() calls per mode")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("source_maps_raygen_bench: needs a GPU (nothing is measured without one)")
    import rnb_neus_fork_amd as R
    dev = torch.device("cuda:0")
    V, H, W, B = args.views, args.height, args.width, args.batch
    normals, albedo, masks, kinv, pose = synthetic_source_maps(V, H, W, dev)
    source = R.DeviceRays.from_source_maps(normals, albedo, masks, kinv, pose, dev)
    mats = [source.materialize(v) for v in range(V)]
    stack = R.DeviceRays(torch.stack([m["images"] for m in mats]), torch.stack([m["images_warmup"] for m in mats]),
                         torch.stack([m["mask"] for m in mats]), torch.stack([m["light_directions"] for m in mats]),
                         source.light_directions_warmup, kinv, pose, dev)
    del mats
    # same capture in both modes: rays bit-equal, colours bit-equal (the stacks are source mode's own values)
    px, py = torch.randint(0, W, (B,), device=dev), torch.randint(0, H, (B,), device=dev)
    a, b = stack.sample(V // 2, B, pixels_x=px, pixels_y=py), source.sample(V // 2, B, pixels_x=px, pixels_y=py)
    same = all(torch.equal(a[k], b[k]) for k in ("rays_o", "rays_d", "near", "far", "mask", "true_rgb", "lights_dir"))
    pixels = V * H * W
    lines = [f"source_maps_raygen_bench: {V} views of {H} x {W} ({pixels} pixels), 3 lights, batch {B}, build "
             f"{R.native.build_id()}, {torch.cuda.get_device_name(0)}; device events around each call, modes alternating "
             f"call by call, views cycling",
             f"{'resident bytes':<28}{'total':>16}{'per pixel':>12}"]
    for name, dr in (("stack", stack), ("source", source)):
        lines.append(f"{name:<28}{dr.resident_bytes():>16d}{dr.resident_bytes() / pixels:>12.3f}")
    lines.append(f"stack / source = {stack.resident_bytes() / source.resident_bytes():.2f} (cameras and warm-up lights, "
                 f"{V * (16 + 16 + 9) * 4} bytes, are in both totals); outputs of one sample() on the same pixels: "
                 f"{'bit-equal' if same else 'DIFFER'}")
    verdicts = []
    for what, n, calls in (
            (f"sample(v, {B})", args.launches, {"stack": lambda i: stack.sample(i % V, B), "source": lambda i: source.sample(i % V, B)}),
            (f"sample(v, {B}, warmup=True)", args.launches, {"stack": lambda i: stack.sample(i % V, B, warmup=True),
                                                            "source": lambda i: source.sample(i % V, B, warmup=True)}),
            (f"view_rays(v) {H} x {W}", args.view_launches, {"stack": lambda i: stack.view_rays(i % V), "source": lambda i: source.view_rays(i % V)})):
        res = timed(calls, n, max(20, n // 10), args.rounds)
        lines.append(f"{what}: {n} timed calls per mode, microseconds")
        lines.append(f"  {'mode':<8}{'median':>10}{'min':>10}{'p90':>10}{'block medians':>50}{'spread':>10}")
        med, spread = {}, {}
        for k, (t, blocks) in res.items():
            med[k], spread[k] = statistics.median(t), max(blocks) - min(blocks)
            p90 = sorted(t)[int(0.9 * (len(t) - 1))]
            lines.append(f"  {k:<8}{med[k]:>10.2f}{min(t):>10.2f}{p90:>10.2f}{' '.join(f'{x:.2f}' for x in blocks):>50}{spread[k]:>10.2f}")
        gap = med["source"] - med["stack"]
        lines.append(f"  source - stack = {gap:+.2f} us; stack mode's own spread {spread['stack']:.2f} us")
        if what.startswith("sample") and "warmup" not in what:
            verdicts.append(f"acceptance ({what}): source is {'within' if gap <= spread['stack'] else 'BEYOND'} stack mode's spread "
                            f"({gap:+.2f} us against {spread['stack']:.2f} us)")
    lines += verdicts
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
