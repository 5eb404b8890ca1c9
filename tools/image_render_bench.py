"""Times one whole-view render (512 x 612, DiLiGenT-MV's image size; synthetic stacks, the shipped network shape at its
seed-0 geometric init) through `NeuSRenderer.render_image` at several `chunk_rays`, and through the only way there was
before it, in the same run:

  loop      rays of the view built with torch ops (Dataset.gen_rays_at's arithmetic on the device), then per 512-ray batch
            near / far in torch, the light gather by torch indexing, `render_rnb` under no_grad, the three torch
            reductions of validate_image (exp_runner.py:460-470) and a `.cpu()` of colour and normals: 612 batches
  image     `render_image(light=, maps=("color", "normal"), to_host=True)`: the same two images, one synchronisation
  image_all `render_image` with its default maps and every light, left on the device

Every configuration renders the same view with the same light; the configurations alternate inside each repetition
(after one warm-up round).  Per configuration: seconds per image (host clock around work that ends in a device
synchronise; median, min, max), rays per second, and the rise of torch.cuda.max_memory_allocated over what was resident
before the call.  The images of `loop` and `image` are compared at the end (with perturb_overwrite=0 for that comparison
only: the timed runs draw their own perturbations).

  python tools/image_render_bench.py --out profiles/image_render.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_rays(dr, v, level=1):
    """Dataset.gen_rays_at (models/dataset.py:300-326) with torch ops on the device"""
    tx = torch.linspace(0, dr.W - 1, dr.W // level, device=dr.device)
    ty = torch.linspace(0, dr.H - 1, dr.H // level, device=dr.device)
    px, py = torch.meshgrid(tx, ty, indexing="ij")
    p = torch.stack([px, py, torch.ones_like(py)], dim=-1)
    p = torch.matmul(dr.intrinsics_all_inv[v, None, None, :3, :3], p[:, :, :, None]).squeeze(-1)
    rays_v = p / torch.linalg.norm(p, ord=2, dim=-1, keepdim=True)
    rays_v = torch.matmul(dr.pose_all[v, None, None, :3, :3], rays_v[:, :, :, None]).squeeze(-1)
    rays_o = dr.pose_all[v, None, None, :3, 3].expand(rays_v.shape)
    return rays_o.transpose(0, 1), rays_v.transpose(0, 1), px.transpose(0, 1), py.transpose(0, 1)


def loop_render(ren, dr, v, light, batch, perturb_overwrite=-1, given=None):
    """validate_image's loop (exp_runner.py:404-470) on the existing entry points (`given`: a `view_rays` dict whose rays,
    near and far are used instead of the torch-built ones)"""
    if given is None:
        rays_o, rays_d, px, py = torch_rays(dr, v)
    else:
        H, W = given["H"], given["W"]
        rays_o, rays_d = given["rays_o"].reshape(H, W, 3), given["rays_d"].reshape(H, W, 3)
        px, py = given["pixels_x"].reshape(H, W), given["pixels_y"].reshape(H, W)
    H, W, _ = rays_o.shape
    px, py = px.round().long().reshape(-1), py.round().long().reshape(-1)
    rays_o, rays_d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
    rgb, nrm = [], []
    with torch.no_grad():
        for i in range(0, H * W, batch):
            o, d = rays_o[i:i + batch], rays_d[i:i + batch]
            if given is None:
                near, far = dr.near_far_from_sphere(o, d)
            else:
                near, far = given["near"][i:i + batch], given["far"][i:i + batch]
            lights = dr.light_directions[v, light, py[i:i + batch], px[i:i + batch], :].unsqueeze(0)
            out = ren.render_rnb(o, d, near, far, lights, perturb_overwrite=perturb_overwrite, cos_anneal_ratio=1.0)
            rgb.append(out["color_fine"].squeeze(0).cpu())
            n = out["gradients"] * out["weights"][:, :, None]
            n = n * out["inside_sphere"][..., None]
            nrm.append(n.sum(dim=1).cpu())
            del out
    return torch.cat(rgb).reshape(H, W, 3), torch.cat(nrm).reshape(H, W, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=612)
    ap.add_argument("--chunks", default="512,1024,2048")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--light", type=int, default=0)
    ap.add_argument("--variant", default="", help="comma-separated set_variant switches, e.g. bf16")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_render_bench: needs a GPU (nothing is measured without one)")
    import rnb_neus_fork_amd as R
    from bench import synthetic_capture
    from oracle import rnb_oracle as O
    dev = torch.device("cuda:0")
    mc = O.ModelConf()
    torch.manual_seed(0)
    sdf, var, col, ren = R.build_from_named_params(mc, O.init_params(mc), dev)
    if args.variant:
        ren.set_variant(**{k: True for k in args.variant.split(",")})
    dr = synthetic_capture(R, dev, 1, args.height, args.width)
    N = args.height * args.width
    S = mc.render.n_samples + mc.render.n_importance
    chunks = [int(c) for c in args.chunks.split(",")]
    default_chunk = R.renderer.DEFAULT_CHUNK_RAYS
    if default_chunk not in chunks:
        chunks.append(default_chunk)
    configs = [("loop 512", lambda: loop_render(ren, dr, 0, args.light, 512))]
    for c in chunks:
        configs.append((f"image {c}", lambda c=c: ren.render_image(dr, 0, light=args.light, cos_anneal_ratio=1.0, chunk_rays=c,
                                                                   maps=("color", "normal"), to_host=True)))
    configs.append((f"image_all {default_chunk}", lambda: ren.render_image(dr, 0, cos_anneal_ratio=1.0)))
    times = {name: [] for name, _ in configs}
    peaks = {}
    for rep in range(args.reps + 1):             # round 0 warms every shape up and is not timed
        for name, fn in configs:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            resident = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            del out
            if rep > 0:
                times[name].append(dt)
                peaks[name] = max(peaks.get(name, 0), torch.cuda.max_memory_allocated() - resident)
    # same images?  Without perturbation and at chunk 512 both ways hand the same batches to the same sampler: on the SAME rays,
    # near and far (view_rays') the depths are equal, the colours are the wrapper's bits and the normals differ by summation
    # order only; on the torch-built rays (directions, near and far a few ulps away) a few importance samples land in a
    # neighbouring bin
    img = ren.render_image(dr, 0, light=args.light, cos_anneal_ratio=1.0, chunk_rays=512, perturb_overwrite=0,
                           maps=("color", "normal"), to_host=True)
    c_same, n_same = loop_render(ren, dr, 0, args.light, 512, perturb_overwrite=0, given=dr.view_rays(0))
    _, n_loop = loop_render(ren, dr, 0, args.light, 512, perturb_overwrite=0)
    got_n, got_c = torch.from_numpy(img["normal"]), torch.from_numpy(img["color"])[0]
    d_same = (got_n - n_same).abs()
    d_loop = (got_n - n_loop).abs()
    lines = [f"image_render_bench: one {args.height} x {args.width} view = {N} rays x {S} samples, 8 x 256 SDF network + albedo "
             f"network, geometric init, light {args.light}, variant '{args.variant or 'default'}', build {R.native.build_id()}, "
             f"{torch.cuda.get_device_name(0)}; {args.reps} timed repetitions after one warm-up round, configurations alternating",
             f"{'configuration':<18}{'s/image (median)':>18}{'min':>9}{'max':>9}{'rays/s':>12}{'peak rise MB':>14}"]
    med = {}
    for name, _ in configs:
        t = times[name]
        med[name] = statistics.median(t)
        lines.append(f"{name:<18}{med[name]:>18.3f}{min(t):>9.3f}{max(t):>9.3f}{N / med[name]:>12.0f}{peaks[name] / 2 ** 20:>14.1f}")
    dflt = f"image {default_chunk}"
    lines.append(f"render_image at its default chunk ({default_chunk}) against the loop: {med['loop 512'] / med[dflt]:.3f} x "
                 f"the loop's speed; peak memory {peaks[dflt] / 2 ** 20:.1f} MB against {peaks['loop 512'] / 2 ** 20:.1f} MB")
    lines.append(f"no perturbation, chunk 512, loop on render_image's own rays, near and far: colour {'bit-equal' if torch.equal(got_c, c_same) else 'DIFFERS'}, "
                 f"normal map max |difference| {float(d_same.max()):.3e}")
    lines.append(f"no perturbation, chunk 512, loop on torch-built rays: normal map max |difference| {float(d_loop.max()):.3e}, "
                 f"{100.0 * float((d_loop.amax(dim=-1) > 1e-5).float().mean()):.2f} % of the pixels beyond 1e-5")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
