"""Times the simplification of a marching-cubes mesh by vertex clustering — at cell sizes of 2, 3 and 4 voxels and to a
target of 100 000 triangles — two ways, and says what each simplification cost in distance:

  (a) device   `simplify_mesh` on the tensors marching cubes left on the GPU (csrc/mesh_simplify.hip): the count stage and
               the emit stage each between two events on the stream (no host read inside), and the whole call, wall-clock
               around a synchronised call, results left on the device; `clean_mesh` with no criteria on the same mesh is
               the yardstick (the same kind of work: a few passes over V and T);
  (b) host     what a user does without it: copy V x 3 doubles and T x 3 ints to the host and run the same definition in
               numpy (tests/mesh_simplify_ref.py);
  (c) distance `mesh_distance` between the original and each result, --samples points per surface: accuracy = result ->
               original (bounded by sqrt(3) h), completeness = original -> result (not bounded: small parts can vanish).

Mesh: the native marching cubes at --res of the analytic volume of tools/mesh_clean_bench.py (a sphere and --floaters small
spheres), or with --sparse of the full_main_sharp fixture's SDF through `extract_fields_sparse`.  Milliseconds: median
[min, max] over --reps blocks of calls (--inner per block for the device), after --warmup blocks.

  python tools/mesh_simplify_bench.py --res 512 --out profiles/mesh_simplify_bench.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wall(fn, reps, warmup, inner):
    """per-call milliseconds around a synchronised block: (median, min, max)"""
    ms = []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            out = fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0) / inner)
        del out
    return statistics.median(ms), min(ms), max(ms)


def _events(fn, reps, warmup, inner):
    """per-call milliseconds between two events on the stream: (median, min, max)"""
    ms = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ms), min(ms), max(ms)


def _fmt(t):
    return f"{t[0]:10.3f} [{t[1]:.3f}, {t[2]:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--sparse", action="store_true", help="the full_main_sharp fixture through extract_fields_sparse")
    ap.add_argument("--floaters", type=int, default=200)
    ap.add_argument("--target", type=int, default=100000)
    ap.add_argument("--samples", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", help="write the report here")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rnb_neus_fork_amd as R
    from rnb_neus_fork_amd import mesh_simplify as MS
    from tests import mesh_simplify_ref as S

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    if a.sparse:
        from tests.golden_util import Golden
        g = Golden("full_main_sharp")
        ren = R.build_from_named_params(g.mc, g.params(), dev)[3]
        lo, hi = torch.tensor([-1.01] * 3), torch.tensor([1.01] * 3)
        u = ren.extract_fields_sparse(lo, hi, a.res, 0.0, to_host=False)[0]
        what = f"full_main_sharp through extract_fields_sparse at res {a.res}"
    else:
        from mesh_clean_bench import floater_volume
        u = floater_volume(a.res, a.floaters, dev)
        what = f"analytic volume at res {a.res}: a sphere + {a.floaters} small spheres"
    v, t = R.marching_cubes(u, 0.0)
    del u
    lines = [f"mesh simplification by vertex clustering; build {R.native.build_id()}; GPU: {torch.cuda.get_device_name(0)}",
             f"{what}; V = {len(v)} vertices, T = {len(t)} triangles (coordinates in voxels)",
             f"ms per call, median [min, max] over {a.reps} blocks after {a.warmup} warm-up blocks; calls per block: device "
             f"{a.inner}, host 1; distances in voxels, {a.samples} samples per surface", ""]
    t_clean = _wall(lambda: R.clean_mesh(v, t), a.reps, a.warmup, a.inner)
    lines.append(f"yardstick: clean_mesh(v, t) with no criteria, whole call           {_fmt(t_clean)}")
    run = MS._Pass("bench", v.contiguous(), t.contiguous())
    lines.append(f"workspace: {run.ws.numel() / 2 ** 20:.1f} MiB")

    def host_route(h):
        vh, th = v.cpu().numpy(), t.cpu().numpy()
        return S.simplify(vh, th, h)

    for h in (2.0, 3.0, 4.0):
        out = R.simplify_mesh(v, t, cell_size=h)
        info = out["info"]
        nv, nt = info["n_vertices"][1], info["n_triangles"][1]
        t_count = _events(lambda: run.launch_count(None, h), a.reps, a.warmup, a.inner)
        run.count(None, h)
        t_emit = _events(lambda: run.emit(nv, nt), a.reps, a.warmup, a.inner)
        t_call = _wall(lambda: R.simplify_mesh(v, t, cell_size=h), a.reps, a.warmup, a.inner)
        want = host_route(h)
        same = all(np.array_equal(out[k].cpu().numpy(), want[k]) for k in ("vertices", "triangles", "vertex_index"))
        t_host_ms = _wall(lambda: host_route(h), min(a.reps, 3), 1, 1)
        d = R.mesh_distance(out["vertices"], out["triangles"], v, t, n_samples=a.samples)
        lines += [f"cell_size = {h:g} voxels: V' = {nv}, T' = {nt} ({100.0 * nt / len(t):.1f} % of T), {info['n_clusters']} clusters, "
                  f"{info['n_degenerate']} degenerate, {info['n_duplicate']} duplicate",
                  f"  (a) count stage, events                                          {_fmt(t_count)}",
                  f"  (a) emit stage (with its five allocations), events               {_fmt(t_emit)}",
                  f"  (a) simplify_mesh, whole call, results on the device             {_fmt(t_call)}",
                  f"      count + emit over clean_mesh, medians                        {(t_count[0] + t_emit[0]) / t_clean[0]:10.2f}",
                  f"  (b) host: copy to host + numpy reference                         {_fmt(t_host_ms)}",
                  f"      host / device whole call, medians                            {t_host_ms[0] / t_call[0]:10.1f}",
                  f"      the two routes give the same arrays: {same}",
                  f"  (c) result -> original: mean {d['accuracy']:.4f}, max {d['max_accuracy']:.4f} (bound sqrt(3) h = "
                  f"{3 ** 0.5 * h:.4f}); original -> result: mean {d['completeness']:.4f}, max {d['max_completeness']:.4f}", ""]
    out = R.simplify_mesh(v, t, target_triangles=a.target)
    info = out["info"]
    t_target = _wall(lambda: R.simplify_mesh(v, t, target_triangles=a.target), a.reps, a.warmup, 2)
    d = R.mesh_distance(out["vertices"], out["triangles"], v, t, n_samples=a.samples)

    def host_target():
        vh, th = v.cpu().numpy(), t.cpu().numpy()
        origin, L = S.target_grid(vh)
        res = None
        for r, _ in info["tried"]:
            res = S.simplify(vh, th, L / r, origin)
        return res

    t_host_target = _wall(host_target, 1, 0, 1)
    lines += [f"target_triangles = {a.target}: T' = {info['n_triangles'][1]}, V' = {info['n_vertices'][1]} at r = {info['resolution']} "
              f"(cell_size {info['cell_size']:.4f} voxels), {len(info['tried'])} count passes",
              f"  tried (r, T'): {info['tried']}",
              f"  (a) simplify_mesh, whole call                                    {_fmt(t_target)}",
              f"  (b) host: the same count passes with the numpy reference, once    {t_host_target[0]:10.1f}",
              f"  (c) result -> original: mean {d['accuracy']:.4f}, max {d['max_accuracy']:.4f}; original -> result: mean "
              f"{d['completeness']:.4f}, max {d['max_completeness']:.4f}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
