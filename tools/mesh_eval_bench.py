"""Times the distance between two meshes — accuracy, completeness, Chamfer — two ways, on the same box:

  (a) device   `mesh_distance`'s stages (csrc/mesh_eval.hip), each between HIP events: build the triangle bins of both
               meshes (`MeshIndex`), draw --samples points on each surface (`sample_surface`), query each sample set
               against the other mesh (`MeshIndex.closest`: point-to-TRIANGLE, exact for the samples drawn);
  (b) host     the usual route without it: the meshes and the samples on the host, `scipy.spatial.cKDTree` over a 4x denser
               resampling of the other surface, nearest POINT for every sample (when scipy imports; else said so).  The
               resampling is drawn by the device sampler and copied: its cost is left out of the host's time, in its favour.

Meshes: `extract_geometry(backend="native", sparse=True)` of the full_main_sharp fixture at --res and at --res-b (default
3/4 of --res): the same surface at two resolutions, in model coordinates.  Milliseconds: median [min, max] over --reps
repetitions after --warmup.  The host's nearest-point distance over-estimates the point-to-triangle distance by up to the
resampling's spacing; the report states both means.

  python tools/mesh_eval_bench.py --res 512 --out profiles/mesh_eval_bench.txt
"""
import argparse
import os
import statistics
import sys
import time

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


def _wall(fn, reps, warmup):
    ms, out = [], None
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        out = fn()
        if k >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    return out, (statistics.median(ms), min(ms), max(ms))


def _fmt(t):
    return f"{t[0]:10.2f} [{t[1]:.2f}, {t[2]:.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--res-b", type=int, default=0, help="resolution of the second mesh (0: 3/4 of --res)")
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--workers", type=int, default=16, help="threads of cKDTree.query")
    ap.add_argument("--out", help="write the report here")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import rnb_neus_fork_amd as R
    from tests.golden_util import Golden

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    g = Golden("full_main_sharp")
    ren = R.build_from_named_params(g.mc, g.params(), dev)[3]
    lo, hi = torch.tensor([-1.01] * 3), torch.tensor([1.01] * 3)
    res_b = a.res_b or a.res * 3 // 4
    meshes = []
    for res in (a.res, res_b):
        v, t = ren.extract_geometry(lo, hi, res, backend="native", sparse=True)
        meshes.append((torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev),
                       torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3)).to(dev)))
    (va, ta), (vb, tb) = meshes
    n = a.samples

    (ia, ib), t_build = _events(lambda: (R.MeshIndex(va, ta), R.MeshIndex(vb, tb)), a.reps, a.warmup)
    (sa, sb), t_sample = _events(lambda: (R.sample_surface(va, ta, n, 0), R.sample_surface(vb, tb, n, 1)), a.reps, a.warmup)
    pa, pb = sa["points"], sb["points"]
    (qa, qb), t_query = _events(lambda: (ib.closest(pa), ia.closest(pb)), a.reps, a.warmup)
    full, t_full = _events(lambda: R.mesh_distance(va, ta, vb, tb, n_samples=n), a.reps, a.warmup)
    lines = [f"mesh-to-mesh distance, {n} samples per surface; build {R.native.build_id()}; GPU: {torch.cuda.get_device_name(0)}",
             f"full_main_sharp, extract_geometry(sparse=True): A at res {a.res}: V = {len(va)}, T = {len(ta)}; "
             f"B at res {res_b}: V = {len(vb)}, T = {len(tb)}",
             f"bins: A {ia.dims} cells, E = {ia.n_entries}; B {ib.dims} cells, E = {ib.n_entries}",
             f"ms, median [min, max] over {a.reps} repetitions after {a.warmup} warm-up; device stages between HIP events", "",
             f"(a) build both indices (bounding box, count, emit; 2 x 2 host reads)   {_fmt(t_build)}",
             f"(a) sample both surfaces (areas, scan, {n} points each)              {_fmt(t_sample)}",
             f"(a) query both ways ({n} point-to-triangle queries each)             {_fmt(t_query)}",
             f"(a) mesh_distance, all of it with the statistics                      {_fmt(t_full)}",
             f"    accuracy {full['accuracy']:.6e}, completeness {full['completeness']:.6e}, chamfer {full['chamfer']:.6e}"]
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
        lines.append("(b) host route: scipy is not importable here: not measured")
    if cKDTree is not None:
        dense_a = R.sample_surface(va, ta, 4 * n, 2)["points"].cpu().numpy()
        dense_b = R.sample_surface(vb, tb, 4 * n, 3)["points"].cpu().numpy()

        def host():
            ha, hb = pa.cpu().numpy(), pb.cpu().numpy()
            da = cKDTree(dense_b).query(ha, workers=a.workers)[0]
            db = cKDTree(dense_a).query(hb, workers=a.workers)[0]
            return float(da.mean()), float(db.mean())

        (acc, comp), t_host = _wall(host, a.host_reps, 0)
        dev_ms = t_build[0] + t_query[0]
        lines += ["", f"(b) host: copy the samples, cKDTree over {4 * n} points of the other surface, query "
                      f"({a.workers} threads), both ways   {_fmt(t_host)}",
                  f"    accuracy {acc:.6e}, completeness {comp:.6e} (nearest resampled POINT: an over-estimate)",
                  f"    host / device (build + query, medians)   {t_host[0] / dev_ms:10.1f}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
