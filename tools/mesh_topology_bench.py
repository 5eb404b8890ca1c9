"""Times the topology audit of a marching-cubes mesh, before and after `simplify_mesh` at 3 voxels, two ways:

  (a) device  the three native stages of `mesh_topology` (csrc/mesh_topology.hip) — count, emit, component table with the
              volume — each between two events on the stream (no host read inside), and the whole call with edges,
              boundary components and components, wall-clock around a synchronised call, results left on the device;
              `clean_mesh` with no criteria on the same mesh gives the scale (the same kind of work: a few passes over V
              and T);
  (b) host    what a user does without it: copy V x 3 doubles and T x 3 ints to the host and run the same definition in
              numpy (tests/mesh_topology_ref.py: np.unique over the 3T edge keys).

Mesh: the native marching cubes at --res of the analytic volume of tools/mesh_clean_bench.py (a sphere and --floaters small
spheres), the mesh tools/mesh_simplify_bench.py builds.  Milliseconds: median [min, max] over --reps blocks of calls
(--inner per block for the device), after --warmup blocks; one process.

  python tools/mesh_topology_bench.py --res 512 --out profiles/mesh_topology_bench.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--floaters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", help="write the report here")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rnb_neus_fork_amd as R
    from mesh_clean_bench import floater_volume
    from mesh_simplify_bench import _events, _fmt, _wall
    from tests import mesh_topology_ref as M

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    N, lib = R.native, R.native.load()
    v0, t0 = R.marching_cubes(floater_volume(a.res, a.floaters, dev), 0.0)
    s = R.simplify_mesh(v0, t0, cell_size=3.0)
    lines = [f"mesh topology audit; build {N.build_id()}; GPU: {torch.cuda.get_device_name(0)}",
             f"analytic volume at res {a.res}: a sphere + {a.floaters} small spheres, through the native marching cubes",
             f"ms per call, median [min, max] over {a.reps} blocks after {a.warmup} warm-up blocks; calls per block: device "
             f"{a.inner}, host 1", ""]
    for name, v, t in (("marching-cubes mesh", v0.contiguous(), t0.contiguous()),
                       ("after simplify_mesh at 3 voxels", s["vertices"].contiguous(), s["triangles"].contiguous())):
        V, T = len(v), len(t)
        rep = R.mesh_topology(t, vertices=v, edges=True)
        E, comp = rep["n_edges"], rep["components"]
        C = comp["n_components"]
        ws = N.workspace("mesh_topology", dev, V, T)
        counts = torch.empty(8, dtype=torch.int64, device=dev)
        tf, vf = torch.empty(T, dtype=torch.uint8, device=dev), torch.empty(V, dtype=torch.uint8, device=dev)
        bl, bd = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev)
        edges, use = torch.empty(E, 2, dtype=torch.int32, device=dev), torch.empty(E, 2, dtype=torch.int32, device=dev)
        etri = torch.empty(E, dtype=torch.int32, device=dev)
        table, vol = torch.empty(C, 8, dtype=torch.int64, device=dev), torch.empty(C, dtype=torch.float64, device=dev)

        def count(boundary=True):
            with N.on_device(dev) as st:
                N.check(lib.rnb_mesh_topology_count(N.ptr(t), T, V, N.ptr(ws), ws.numel(), N.ptr(counts), N.ptr(tf), N.ptr(vf),
                                                    N.ptr(bl) if boundary else None, N.ptr(bd) if boundary else None, st))

        def emit():
            with N.on_device(dev) as st:
                N.check(lib.rnb_mesh_topology_emit(N.ptr(t), T, V, N.ptr(ws), ws.numel(), E, N.ptr(edges), N.ptr(use),
                                                   N.ptr(etri), st))

        def table_of(with_volume=True):
            with N.on_device(dev) as st:
                N.check(lib.rnb_mesh_topology_components(N.ptr(t), T, N.ptr(v) if with_volume else None, V, N.ptr(comp["labels"]),
                                                         C, N.ptr(ws), ws.numel(), N.ptr(table),
                                                         N.ptr(vol) if with_volume else None, st))

        args = (a.reps, a.warmup, a.inner)
        t_count, t_count_nb = _events(count, *args), _events(lambda: count(False), *args)
        count()
        t_emit, t_table, t_table_nv = _events(emit, *args), _events(table_of, *args), _events(lambda: table_of(False), *args)
        t_call = _wall(lambda: R.mesh_topology(t, vertices=v, edges=True), *args)
        t_lean = _wall(lambda: R.mesh_topology(t, V, boundary=False, components=False), *args)
        t_clean = _wall(lambda: R.clean_mesh(v, t), *args)

        def host_route():
            return M.topology(t.cpu().numpy(), V, v.cpu().numpy())

        want = host_route()
        same = (np.array_equal(rep["edges"].cpu().numpy(), want["edges"]) and np.array_equal(rep["edge_use"].cpu().numpy(), want["edge_use"])
                and np.array_equal(rep["boundary_labels"].cpu().numpy(), want["boundary_labels"])
                and [rep[k] for k in ("n_edges", "n_boundary", "n_manifold", "n_flipped", "n_nonmanifold")] == want["counts"][:5].tolist())
        t_host = _wall(host_route, min(a.reps, 3), 1, 1)
        lines += [f"{name}: V = {V}, T = {T}, E = {E}; boundary {rep['n_boundary']}, flipped {rep['n_flipped']}, non-manifold "
                  f"{rep['n_nonmanifold']} edges, {rep['n_degenerate']} degenerate triangles, {rep['n_boundary_components']} boundary "
                  f"components, {C} components ({int(comp['closed'].sum())} closed); workspace {ws.numel() / 2 ** 20:.1f} MiB",
                  f"  (a) count stage, events                                          {_fmt(t_count)}",
                  f"      count stage without boundary components, events              {_fmt(t_count_nb)}",
                  f"  (a) emit stage, events                                           {_fmt(t_emit)}",
                  f"  (a) component table with the volume, events                      {_fmt(t_table)}",
                  f"      component table without coordinates, events                  {_fmt(t_table_nv)}",
                  f"  (a) mesh_topology, everything, whole call, results on the device {_fmt(t_call)}",
                  f"      mesh_topology, counts and flags only, whole call             {_fmt(t_lean)}",
                  f"      clean_mesh(v, t) with no criteria, whole call                {_fmt(t_clean)}",
                  f"      the three stages over clean_mesh, medians                    {(t_count[0] + t_emit[0] + t_table[0]) / t_clean[0]:10.2f}",
                  f"  (b) host: copy to host + numpy reference                         {_fmt(t_host)}",
                  f"      host / device whole call, medians                            {t_host[0] / t_call[0]:10.1f}",
                  f"      the two routes give the same arrays: {same}", ""]
        del ws, edges, use, etri
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
