"""Times what a camera sees of a mesh — `MeshIndex.raycast` (csrc/mesh_raycast.hip) — on two kinds of rays:

  (a) coherent    one 512 x 612 view, every ray of `DeviceRays.view_rays` (a camera on the radius-3 sphere whose field of
                  view just holds the unit sphere), against the default bins; `mesh_view_maps` of the same view with
                  interpolated normals; and, as the figure a user would otherwise pay, one `render_image` normal map of
                  the same view through the volume renderer (the field, not the mesh);
  (b) incoherent  --segments segments between area-weighted samples of the surface, shuffled (the rays of a visibility
                  or occlusion query), in the order given and sorted by the cell of their origin as `MeshIndex.closest`
                  sorts its queries (which is why `raycast` does not sort: the two numbers are the reason).

Both against `cells=1`, brute force over every triangle, on a subsample of --brute rays — whose answers must equal the
default grid's bit for bit, and the tool says whether they do.

Mesh: `extract_geometry(backend="native", sparse=True)` of the full_main_sharp fixture at --res, in model coordinates.
Milliseconds between HIP events: median [min, max] over --reps repetitions after --warmup.  With --codegen (hipcc on the
path) the kernel's registers and scratch are read from -Rpass-analysis=kernel-resource-usage and reported too.

  python tools/mesh_raycast_bench.py --res 512 --codegen --out profiles/mesh_raycast_bench.txt
"""
import argparse
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _events(fn, reps, warmup):
    """(result of the last call, (median, min, max) ms between two HIP events around fn())"""
    ms, out = [], None
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    return out, (statistics.median(ms), min(ms), max(ms))


def _fmt(t):
    return f"{t[0]:10.3f} [{t[1]:.3f}, {t[2]:.3f}]"


def _same(a, b):
    return all(torch.equal(torch.nan_to_num(a[k], nan=-7.0), torch.nan_to_num(b[k], nan=-7.0)) for k in ("t", "triangle", "bary"))


def kernel_resources():
    """one line from hipcc -Rpass-analysis=kernel-resource-usage on csrc/mesh_raycast.hip with the build's flags"""
    from rnb_neus_fork_amd import buildid
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "rnb-neus-fork_amd", "csrc", "mesh_raycast.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc] + buildid.COMMON_FLAGS + buildid.EXTRA_FLAGS["mesh_raycast.hip"] + [
            "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "x.o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return f"kernel resources: hipcc failed ({r.stderr.strip().splitlines()[-1] if r.stderr.strip() else r.returncode})"
    got = {k: re.search(re.escape(k) + r":\s*(\S+)", r.stderr) for k in
           ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")}
    return ("rc_kernel (" + " ".join(buildid.COMMON_FLAGS[:2] + buildid.EXTRA_FLAGS["mesh_raycast.hip"]) + ", kernel-resource-usage): "
            + ", ".join(f"{k} {m.group(1) if m else '?'}" for k, m in got.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=612)
    ap.add_argument("--segments", type=int, default=1_000_000)
    ap.add_argument("--brute", type=int, default=4096, help="rays of each kind sent to the one-cell grid as well")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-render", action="store_true", help="skip the render_image comparison")
    ap.add_argument("--codegen", action="store_true", help="report the kernel's registers and scratch (needs hipcc)")
    ap.add_argument("--out", help="write the report here")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import rnb_neus_fork_amd as R
    from bench import synthetic_capture
    from tests.golden_util import Golden

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    g = Golden("full_main_sharp")
    ren = R.build_from_named_params(g.mc, g.params(), dev)[3]
    v, t = ren.extract_geometry(torch.tensor([-1.01] * 3), torch.tensor([1.01] * 3), a.res, backend="native", sparse=True)
    v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)
    t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3)).to(dev)
    index, t_build = _events(lambda: R.MeshIndex(v, t), a.reps, a.warmup)
    brute = R.MeshIndex(v, t, cells=1)
    dr = synthetic_capture(R, dev, 1, a.height, a.width)
    rays = dr.view_rays(0)
    ro, rd = rays["rays_o"].double().contiguous(), rays["rays_d"].double().contiguous()
    n_view = ro.shape[0]
    vn = torch.nn.functional.normalize(v, dim=1)                  # stand-in per-vertex normals: the cost is the same

    hits, t_view = _events(lambda: index.raycast(ro, rd), a.reps, a.warmup)
    _, t_view32 = _events(lambda: index.raycast(rays["rays_o"], rays["rays_d"]), a.reps, a.warmup)
    _, t_maps = _events(lambda: R.mesh_view_maps(index, rays, vertex_normals=vn), a.reps, a.warmup)
    sub = torch.arange(0, n_view, max(n_view // a.brute, 1), device=dev)
    bv, t_bview = _events(lambda: brute.raycast(ro[sub], rd[sub]), max(a.reps // 2, 1), 1)
    gv, t_gview = _events(lambda: index.raycast(ro[sub], rd[sub]), a.reps, a.warmup)

    n = a.segments
    p = R.sample_surface(v, t, n, 0)["points"]
    q = R.sample_surface(v, t, n, 1)["points"][torch.randperm(n, generator=torch.Generator().manual_seed(0)).to(dev)]
    so, sd = p.contiguous(), (q - p).contiguous()
    seg, t_seg = _events(lambda: index.raycast(so, sd, 0.0, 1.0), a.reps, a.warmup)

    def sorted_cast():
        """what `MeshIndex.closest` does for its queries: the rays in the order of their origins' cells, results scattered back"""
        order = index._cell_order(so)
        out = index.raycast(so.index_select(0, order), sd.index_select(0, order), 0.0, 1.0)
        back = {k: torch.empty_like(out[k]) for k in ("t", "triangle", "bary")}
        for k in back:
            back[k][order] = out[k]
        return back

    seg_s, t_seg_sorted = _events(sorted_cast, a.reps, a.warmup)
    _, t_visible = _events(lambda: index.visible(q, p), a.reps, a.warmup)
    ssub = torch.arange(0, n, max(n // a.brute, 1), device=dev)
    bs, t_bseg = _events(lambda: brute.raycast(so[ssub], sd[ssub], 0.0, 1.0), max(a.reps // 2, 1), 1)
    gs, t_gseg = _events(lambda: index.raycast(so[ssub], sd[ssub], 0.0, 1.0), a.reps, a.warmup)

    lines = [f"mesh ray casting; build {R.native.build_id()}; GPU: {torch.cuda.get_device_name(0)}",
             f"full_main_sharp, extract_geometry(sparse=True) at res {a.res}: V = {len(v)}, T = {len(t)}; bins {index.dims} cells, "
             f"E = {index.n_entries}",
             f"ms between HIP events, median [min, max] over {a.reps} repetitions after {a.warmup} warm-up", "",
             f"build the index (bounding box, count, emit)                                   {_fmt(t_build)}",
             f"(a) one {a.height} x {a.width} view = {n_view} rays of view_rays, float64 rays, raycast       {_fmt(t_view)}",
             f"    {int(hits['hit'].sum())} rays hit ({100.0 * float(hits['hit'].double().mean()):.1f} %); {n_view / t_view[0] / 1e3:.1f} M rays/s",
             f"(a) the same from the float32 rays of view_rays (widened on the way)          {_fmt(t_view32)}",
             f"(a) mesh_view_maps of the view with interpolated normals                      {_fmt(t_maps)}",
             f"(a) {len(sub)} of those rays: default grid                                    {_fmt(t_gview)}",
             f"(a) {len(sub)} of those rays: cells=1, brute force over {len(t)} triangles    {_fmt(t_bview)}",
             f"    default grid and brute force bit-equal: {_same(bv, gv)}", "",
             f"(b) {n} shuffled segments between surface samples, t in [0, 1], unsorted      {_fmt(t_seg)}",
             f"    {int(seg['hit'].sum())} segments meet the mesh; {n / t_seg[0] / 1e3:.1f} M rays/s",
             f"(b) the same sorted by origin cell (argsort, gather, scatter included)        {_fmt(t_seg_sorted)}",
             f"    sorted and unsorted bit-equal: {_same(seg, seg_s)}",
             f"(b) MeshIndex.visible(points, eye per point) of the same segments              {_fmt(t_visible)}",
             f"(b) {len(ssub)} of those segments: default grid                               {_fmt(t_gseg)}",
             f"(b) {len(ssub)} of those segments: cells=1, brute force                       {_fmt(t_bseg)}",
             f"    default grid and brute force bit-equal: {_same(bs, gs)}"]
    if not a.no_render:
        _, t_render = _events(lambda: ren.render_image(dr, 0, light=0, cos_anneal_ratio=1.0, maps=("normal",)), max(a.reps // 2, 1), 1)
        lines += ["", f"render_image(maps=('normal',)) of the same view through the volume renderer    {_fmt(t_render)}",
                  f"    render_image / (raycast + maps, medians)   {t_render[0] / t_maps[0]:10.1f}"]
    if a.codegen:
        lines += ["", kernel_resources()]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
