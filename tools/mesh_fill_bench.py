"""Times the hole filling of a marching-cubes mesh with holes, two ways:

  (a) device  `boundary_loops` and `fill_holes` (csrc/mesh_fill.hip), each as a whole call, wall-clock around a synchronised
              call with the results left on the device, and stage by stage between two events on the stream (no host read
              inside): the audit's count (which builds the edge table the loops are read from), the loop count, the loop
              emit (the ranking: pointer jumping, and the placement), the centroids, the fill emit.  `mesh_topology` on the
              same mesh, which shares the table build, gives the scale;
  (b) host    what a user does without it: copy V x 3 doubles and T x 3 ints to the host and run the same definition in
              numpy / Python (tests/mesh_fill_ref.py).

Mesh: the native marching cubes at --res of the analytic volume of tools/mesh_clean_bench.py (a sphere and --floaters small
spheres) with --removed random triangles taken out (no cameras are at hand for a cull).  Then the evidence that no walk is
serial in the loop's length: the loop emit on one ring of 2^17 + 3 edges against one of 2^10 (an open tube of two rings).
Milliseconds: median [min, max] over --reps blocks of calls (--inner per block for the device), after --warmup blocks.

  python tools/mesh_fill_bench.py --res 512 --out profiles/mesh_fill_bench.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--floaters", type=int, default=200)
    ap.add_argument("--removed", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the host route (minutes at res 512)")
    ap.add_argument("--out", help="write the report here")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rnb_neus_fork_amd as R
    from mesh_clean_bench import floater_volume
    from mesh_simplify_bench import _events, _fmt, _wall
    from tests import mesh_fill_ref as F

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    N, lib = R.native, R.native.load()
    args = (a.reps, a.warmup, a.inner)

    def stages(v, t):
        """per-stage event times of one mesh, and the dict of the whole call"""
        V, T = len(v), len(t)
        tws, ws = N.workspace("mesh_topology", dev, V, T), N.workspace("mesh_fill", dev, V, T)
        tc, c = torch.empty(8, dtype=torch.int64, device=dev), torch.empty(16, dtype=torch.int64, device=dev)
        tf, vf = torch.empty(T, dtype=torch.uint8, device=dev), torch.empty(V, dtype=torch.uint8, device=dev)
        bl, bd = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev)

        def audit_count():
            with N.on_device(dev) as st:
                N.check(lib.rnb_mesh_topology_count(N.ptr(t), T, V, N.ptr(tws), tws.numel(), N.ptr(tc), N.ptr(tf), N.ptr(vf),
                                                    N.ptr(bl), N.ptr(bd), st))

        def loops_count():
            with N.on_device(dev) as st:
                N.check(lib.rnb_mesh_loops_count(T, V, N.ptr(tws), tws.numel(), N.ptr(bl), N.ptr(bd), -1, N.ptr(ws), ws.numel(),
                                                 N.ptr(c), st))

        audit_count()
        loops_count()
        h = [int(x) for x in c.cpu()]
        L, B, Fn, Nn, longest, unwalked = h[0], h[1], h[2], h[3], h[8], h[9]
        off, lv = torch.empty(L + 1, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        status, edges = torch.empty(L, dtype=torch.uint8, device=dev), torch.empty(L, dtype=torch.int32, device=dev)
        cen = torch.empty(L, 3, dtype=torch.float64, device=dev)
        vo, to = torch.empty(V + Fn, 3, dtype=torch.float64, device=dev), torch.empty(T + Nn, 3, dtype=torch.int32, device=dev)
        fl = torch.empty(Fn, dtype=torch.int32, device=dev)

        def loops_emit():
            with N.on_device(dev) as st:
                N.check(lib.rnb_mesh_loops_emit(T, V, N.ptr(bl), N.ptr(ws), ws.numel(), L, B, longest, unwalked, N.ptr(off), N.ptr(lv),
                                                N.ptr(status), N.ptr(edges), st))

        def centroids():
            with N.on_device(dev) as st:
                N.check(lib.rnb_mesh_loops_mean(N.ptr(v), 0, V, 3, N.ptr(off), N.ptr(lv), L, B, N.ptr(ws), ws.numel(), N.ptr(cen), st))

        def fill_emit():
            with N.on_device(dev) as st:
                N.check(lib.rnb_mesh_fill_emit(N.ptr(v), V, N.ptr(t), T, N.ptr(off), N.ptr(lv), N.ptr(status), N.ptr(cen), L, B, -1,
                                               N.ptr(ws), ws.numel(), Fn, Nn, N.ptr(vo), N.ptr(to), N.ptr(fl), st))

        times = {"audit count": _events(audit_count, *args), "loop count": _events(loops_count, *args)}
        loops_emit()
        centroids()
        times.update({"loop emit": _events(loops_emit, *args), "centroids": _events(centroids, *args),
                      "fill emit": _events(fill_emit, *args)})
        rounds = max(longest - 1, 0).bit_length()
        return times, dict(L=L, B=B, F=Fn, N=Nn, longest=longest, unwalked=unwalked, rounds=rounds,
                           ws=(tws.numel() + ws.numel()) / 2 ** 20)

    v0, t0 = R.marching_cubes(floater_volume(a.res, a.floaters, dev), 0.0)
    keep = torch.ones(len(t0), dtype=torch.bool)
    keep[torch.from_numpy(np.random.default_rng(11).choice(len(t0), min(a.removed, len(t0) // 2), replace=False))] = False
    v, t = v0.contiguous(), t0[keep.to(dev)].contiguous()
    V, T = len(v), len(t)
    lines = [f"mesh hole filling; build {N.build_id()}; GPU: {torch.cuda.get_device_name(0)}",
             f"analytic volume at res {a.res}: a sphere + {a.floaters} small spheres, through the native marching cubes, "
             f"{len(t0) - T} random triangles removed",
             f"ms per call, median [min, max] over {a.reps} blocks after {a.warmup} warm-up blocks; calls per block: device "
             f"{a.inner}; the host route runs once", ""]
    times, n = stages(v, t)
    out = R.fill_holes(v, t)
    info = out["info"]
    after = R.mesh_topology(out["triangles"], vertices=out["vertices"])
    t_loops = _wall(lambda: R.boundary_loops(t, vertices=v), *args)
    t_fill = _wall(lambda: R.fill_holes(v, t), *args)
    t_top = _wall(lambda: R.mesh_topology(t, vertices=v), *args)
    lines += [f"V = {V}, T = {T}: {n['L']} loops over {n['B']} boundary vertices, longest simple loop {n['longest']} ({n['rounds']} "
              f"rounds), {n['unwalked']} vertices on loops that are not walked; workspaces {n['ws']:.1f} MiB",
              f"  info {info}",
              f"  after the fill: {after['n_boundary']} boundary edges in {after['n_boundary_components']} loops, watertight "
              f"{R.watertight(after)}"]
    for k, x in times.items():
        lines.append(f"  (a) {k + ', events':58s} {_fmt(x)}")
    lines += [f"  (a) {'boundary_loops with centroids, whole call':58s} {_fmt(t_loops)}",
              f"  (a) {'fill_holes, whole call, results on the device':58s} {_fmt(t_fill)}",
              f"      {'mesh_topology with components and volume, whole call':58s} {_fmt(t_top)}"]
    if not a.no_host:
        def host_route():
            return F.fill(v.cpu().numpy(), t.cpu().numpy())

        torch.cuda.synchronize()
        h0 = time.perf_counter()
        want = host_route()
        t_host = (1e3 * (time.perf_counter() - h0),) * 3         # (one run: seconds of Python)
        same = (np.array_equal(out["triangles"].cpu().numpy(), want["triangles"]) and info == want["info"]
                and np.array_equal(out["filled"].cpu().numpy(), want["filled"]))
        got_c = out["vertices"][V:].cpu().numpy()
        ref_c = want["vertices"][V:]
        vh = v.cpu().numpy()
        bound = np.array([F.mean_bound(vh, want["loops"]["_members"][l]) for l in want["filled"]]).reshape(-1, 3)
        ratio = float((np.abs(got_c - ref_c) / bound).max()) if len(bound) else 0.0
        lines += [f"  (b) {'host: copy to host + the reference in numpy / Python':58s} {_fmt(t_host)}",
                  f"      host / device whole call, medians                          {t_host[0] / t_fill[0]:10.1f}",
                  f"      the two routes give the same triangles, filled and info: {same}",
                  f"      largest centroid error over the bound n 2^-52 mean|x|: {ratio:.3f}"]
    lines.append("")
    ring = {}
    for n_edges in (2 ** 10, 2 ** 17 + 3):
        rv, rt = (torch.from_numpy(x).to(dev) for x in F.tube(n_edges, 2))
        ring[n_edges], m = stages(rv, rt)
        lines.append(f"one ring of {n_edges} edges (a tube of two rings: two loops), {m['rounds']} rounds: "
                     f"loop emit {_fmt(ring[n_edges]['loop emit'])}; loop count {_fmt(ring[n_edges]['loop count'])}; "
                     f"centroids {_fmt(ring[n_edges]['centroids'])}")
    small, large = ring[2 ** 10]["loop emit"][0], ring[2 ** 17 + 3]["loop emit"][0]
    lines += [f"loop emit, long ring over short ring, medians: {large / small:.2f} (the lengths' ratio is {(2 ** 17 + 3) / 2 ** 10:.1f})", ""]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
