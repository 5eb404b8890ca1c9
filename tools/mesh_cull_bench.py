"""Times the culling of a mesh by its cameras — `MeshIndex.view_votes` (csrc/mesh_cull.hip), `compact_triangles`
(csrc/mesh_clean.hip) and `cull_mesh` end to end — against the route a user composed before they existed:

  fused     one `view_votes` launch for all cameras; `compact_triangles` on the device; `cull_mesh` = both plus the keep;
  composed  per view: the projection and the mask gather as torch ops (in the kernel's operation order, so that the two
            routes can be held to identical votes), `MeshIndex.visible(points, eye)` for EVERY point — the segment cast has
            no way to skip the pairs the mask rejects — and torch counting; then the compaction in numpy on the host.

The tool ASSERTS that both routes give identical votes and the same culled mesh.  The two routes are timed alternately,
repetition by repetition, in one process.

Mesh: `extract_geometry(backend="native", sparse=True)` of the full_main_sharp fixture at --res, in model coordinates.
Cameras: a ring of --views synthetic cameras of --height x --width pixels on the radius-3 sphere (alternating elevations),
whose field of view just holds the unit sphere; masks: the mesh's own silhouettes from `mesh_view_maps`, dilated by
--dilate pixels.  Milliseconds between HIP events: median [min, max] over --reps repetitions after --warmup.  With --codegen
(hipcc on the path) the kernels' registers and scratch are read from -Rpass-analysis=kernel-resource-usage.

  python tools/mesh_cull_bench.py --res 512 --codegen --out profiles/mesh_cull_bench.txt
"""
import argparse
import math
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


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def _alternate(fns, reps, warmup):
    """{name: (last result, (median, min, max) ms)} of several callables run in turn, repetition by repetition"""
    ms, out = {k: [] for k in fns}, {}
    for r in range(warmup + reps):
        for k, fn in fns.items():
            out[k], t = _timed(fn)
            if r >= warmup:
                ms[k].append(t)
    return {k: (out[k], (statistics.median(ms[k]), min(ms[k]), max(ms[k]))) for k in fns}


def _fmt(t):
    return f"{t[0]:10.3f} [{t[1]:.3f}, {t[2]:.3f}]"


def ring_cameras(n, H, W):
    """(intrinsics_inv [n,4,4], pose [n,4,4]) float64 numpy: eyes on the radius-3 sphere, azimuths evenly spread,
    elevations alternating between +-25 degrees, looking at the origin (x right, y down, z forward)"""
    focal = 0.5 * min(H, W) / math.tan(math.asin(1.0 / 3.0))
    K = np.eye(4)
    K[0, 0] = K[1, 1] = focal
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    pose = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        az, el = 2.0 * math.pi * k / n, math.radians(25.0 if k % 2 == 0 else -25.0)
        eye = 3.0 * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(fwd, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        pose[k, :3, 0], pose[k, :3, 1], pose[k, :3, 2], pose[k, :3, 3] = right, np.cross(fwd, right), fwd, eye
    return np.tile(np.linalg.inv(K), (n, 1, 1)), pose


def silhouettes(R, index, kinv, pose, H, W, dilate):
    """[n,H,W] uint8: where the rays Kinv (x, y, 1) of every camera meet the mesh (`mesh_view_maps`), dilated"""
    dev = index.device
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    pix = torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(H * W, dtype=torch.float64, device=dev)], dim=1)
    out = []
    for k in range(len(pose)):
        d = pix @ torch.from_numpy(kinv[k, :3, :3].T.copy()).to(dev) @ torch.from_numpy(pose[k, :3, :3].T.copy()).to(dev)
        o = torch.from_numpy(pose[k, :3, 3].copy()).to(dev).expand_as(d).contiguous()
        out.append(R.mesh_view_maps(index, o, d.contiguous(), shape=(H, W))["mask"].to(torch.float32))
    return R.binary_masks(torch.stack(out), dilate=dilate)


def composed_votes(index, pts, P, eyes, masks):
    """The votes on the entry points the package had before `view_votes`: per view a torch projection (the kernel's
    operation order), a mask gather, `MeshIndex.visible` for every point, torch counting.  (counts [N,4] int32, the
    per-view share of pairs that reach the cast as a device tensor [C])"""
    n_cam, H, W = masks.shape
    X, Y, Z = pts[:, 0], pts[:, 1], pts[:, 2]
    fin = torch.isfinite(pts).all(dim=1)
    counts = torch.zeros(pts.shape[0], 4, dtype=torch.int32, device=pts.device)
    share = []
    for c in range(n_cam):
        p = P[c]
        x, y, w = (((p[r, 0] * X + p[r, 1] * Y) + p[r, 2] * Z) + p[r, 3] for r in range(3))
        a, b = x / w + 0.5, y / w + 0.5
        inside = fin & torch.isfinite(w) & (w > 0.0) & (a >= 0.0) & (a < float(W)) & (b >= 0.0) & (b < float(H))
        px = torch.where(inside, torch.floor(a), torch.zeros_like(a)).to(torch.int64)
        py = torch.where(inside, torch.floor(b), torch.zeros_like(b)).to(torch.int64)
        in_mask = masks[c][py, px] != 0
        vis = index.visible(pts, eyes[c])
        status = torch.where(inside, torch.where(in_mask, torch.where(vis, 3, 2), 1), 0)
        counts += torch.nn.functional.one_hot(status, 4).to(torch.int32)
        share.append((inside & in_mask).to(torch.float64).mean())
    return counts, torch.stack(share)


def keep_of(counts, triangles, max_outside=0, min_seen=1):
    keep_v = (counts[:, 1] <= max_outside) & (counts[:, 3] >= min_seen)
    return keep_v[triangles.to(torch.int64)].all(dim=1)


def host_compaction(vertices, triangles, keep_t):
    """the compaction a user wrote in numpy: the arrays go to the host, the culled mesh stays there"""
    v, t, k = vertices.cpu().numpy(), triangles.cpu().numpy(), keep_t.cpu().numpy()
    kept = t[k]
    used = np.zeros(len(v), dtype=bool)
    used[kept.reshape(-1)] = True
    new = np.cumsum(used, dtype=np.int64) - 1
    return v[used], new[kept].astype(np.int32), np.flatnonzero(used), np.flatnonzero(k)


def kernel_resources(src, kernel):
    """one line from hipcc -Rpass-analysis=kernel-resource-usage on a source of csrc/ with the build's flags"""
    from rnb_neus_fork_amd import buildid
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    path = os.path.join(ROOT, "rnb-neus-fork_amd", "csrc", src)
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc] + buildid.COMMON_FLAGS + buildid.EXTRA_FLAGS[src] + ["-Rpass-analysis=kernel-resource-usage", "-c", path, "-o",
                                                                           os.path.join(tmp, "x.o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return f"{kernel}: hipcc failed ({r.stderr.strip().splitlines()[-1] if r.stderr.strip() else r.returncode})"
    block = r.stderr.split("Function Name: ")
    mine = next((b for b in block if kernel in b.splitlines()[0]), "")
    got = {k: re.search(re.escape(k) + r":\s*(\S+)", mine) for k in
           ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")}
    return (f"{kernel} ({src}; " + " ".join(buildid.COMMON_FLAGS[:2] + buildid.EXTRA_FLAGS[src]) + ", kernel-resource-usage): "
            + ", ".join(f"{k} {m.group(1) if m else '?'}" for k, m in got.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=612)
    ap.add_argument("--dilate", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--codegen", action="store_true", help="report the kernels' registers and scratch (needs hipcc)")
    ap.add_argument("--out", help="write the report here")
    a = ap.parse_args()
    assert a.reps >= 5, "the medians are taken over at least 5 repetitions"
    sys.path.insert(0, ROOT)
    import rnb_neus_fork_amd as R
    from tests.golden_util import Golden

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    g = Golden("full_main_sharp")
    ren = R.build_from_named_params(g.mc, g.params(), dev)[3]
    v, t = ren.extract_geometry(torch.tensor([-1.01] * 3), torch.tensor([1.01] * 3), a.res, backend="native", sparse=True)
    v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)
    t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3)).to(dev)
    index = R.MeshIndex(v, t)
    H, W = a.height, a.width
    kinv, pose = ring_cameras(a.views, H, W)
    P, eyes = (x.to(dev) for x in R.camera_projections(kinv, pose))
    masks = silhouettes(R, index, kinv, pose, H, W, a.dilate)
    images = masks * 255          # the mask IMAGES cull_mesh takes (it binarises them itself)

    votes = _alternate({"fused": lambda: index.view_votes(v, P, eyes, masks)["counts"],
                        "composed": lambda: composed_votes(index, v, P, eyes, masks)}, a.reps, a.warmup)
    fused, (composed, share) = votes["fused"][0], votes["composed"][0]
    assert torch.equal(fused, composed), "the fused launch and the composed route disagree on the votes"
    assert bool((fused.sum(dim=1) == a.views).all())
    keep_t = keep_of(fused, t)
    comp = _alternate({"fused": lambda: R.compact_triangles(v, t, keep_t), "composed": lambda: host_compaction(v, t, keep_t)}, a.reps, a.warmup)
    dv, hv = comp["fused"][0], comp["composed"][0]
    assert np.array_equal(dv["vertices"].cpu().numpy(), hv[0]) and np.array_equal(dv["triangles"].cpu().numpy(), hv[1])
    assert np.array_equal(dv["vertex_index"].cpu().numpy(), hv[2]) and np.array_equal(dv["triangle_index"].cpu().numpy(), hv[3])

    def composed_cull():
        counts = composed_votes(index, v, P, eyes, masks)[0]
        return host_compaction(v, t, keep_of(counts, t))

    ends = _alternate({"fused": lambda: R.cull_mesh(v, t, projections=P, eyes=eyes, masks=images, index=index),
                       "fused + index": lambda: R.cull_mesh(v, t, projections=P, eyes=eyes, masks=images),
                       "composed": composed_cull}, a.reps, a.warmup)
    culled, hc = ends["fused"][0], ends["composed"][0]
    assert np.array_equal(culled["vertices"].cpu().numpy(), hc[0]) and np.array_equal(culled["triangles"].cpu().numpy(), hc[1])
    assert torch.equal(culled["info"]["votes"], fused)
    noocc = _alternate({"no occlusion": lambda: index.view_votes(v, P, eyes, masks, occlusion=False)["counts"],
                        "with status": lambda: index.view_votes(v, P, eyes, masks, return_status=True)["counts"]}, a.reps, a.warmup)

    share = share.cpu().numpy()
    hist = np.bincount(fused[:, 3].cpu().numpy(), minlength=a.views + 1)
    N, n_pairs = len(v), len(v) * a.views

    def verdict(f, c):
        return (f"fused median {f[0]:.3f} ms vs composed best run {c[1]:.3f} ms: "
                + ("TARGET MET" if f[0] < c[1] else "TARGET MISSED") + f" ({c[1] / f[0]:.2f} x)")

    lines = [f"mesh culling by the cameras; build {R.native.build_id()}; GPU: {torch.cuda.get_device_name(0)}",
             f"full_main_sharp, extract_geometry(sparse=True) at res {a.res}: V = {N}, T = {len(t)}; bins {index.dims} cells, E = {index.n_entries}",
             f"{a.views} cameras of {H} x {W} on a ring of radius 3 (elevations +-25 degrees); masks: the mesh's silhouettes dilated by {a.dilate} px",
             f"ms between HIP events, median [min, max] over {a.reps} repetitions after {a.warmup} warm-up; the routes alternate, repetition by repetition",
             f"target: the fused route's median below the composed route's BEST run", "",
             f"votes, {n_pairs} pairs: view_votes, ONE launch                                   {_fmt(votes['fused'][1])}",
             f"votes: composed (torch projection + mask gather + visible per view + counting)   {_fmt(votes['composed'][1])}",
             f"    identical votes: True (asserted);  {verdict(votes['fused'][1], votes['composed'][1])}",
             f"    {n_pairs / votes['fused'][1][0] / 1e3:.1f} M pairs/s fused; pairs that reach the cast, per view: mean {100 * share.mean():.1f} %, "
             f"min {100 * share.min():.1f} %, max {100 * share.max():.1f} % (the composed route casts 100 %)",
             f"    vertices by the number of cameras that see them (0 .. {a.views}): {hist.tolist()}",
             f"votes without occlusion (projection + mask only)                                 {_fmt(noocc['no occlusion'][1])}",
             f"votes with the status array [C,N]                                                {_fmt(noocc['with status'][1])}", "",
             f"compaction to {culled['info']['n_triangles'][1]} of {len(t)} triangles, {culled['info']['n_vertices'][1]} of {N} vertices: "
             f"compact_triangles                    {_fmt(comp['fused'][1])}",
             f"compaction: composed (arrays to the host, numpy)                                 {_fmt(comp['composed'][1])}",
             f"    identical meshes: True (asserted);  {verdict(comp['fused'][1], comp['composed'][1])}", "",
             f"cull_mesh end to end on a given index (masks binarised, votes, keep, compaction) {_fmt(ends['fused'][1])}",
             f"cull_mesh end to end, building its MeshIndex                                     {_fmt(ends['fused + index'][1])}",
             f"composed end to end on a given index (votes, keep, numpy compaction)             {_fmt(ends['composed'][1])}",
             f"    identical meshes: True (asserted);  {verdict(ends['fused'][1], ends['composed'][1])}"]
    if a.codegen:
        lines += ["", kernel_resources("mesh_cull.hip", "cv_kernel"), kernel_resources("mesh_raycast.hip", "rc_kernel")]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
