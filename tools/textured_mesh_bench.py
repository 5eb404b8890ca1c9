"""Times the per-vertex attribute stage of a textured mesh two ways, on the same model and the same vertices:

  native     `NeuSRenderer.vertex_attributes(grid_vertices=...)` — the stage `extract_textured_geometry` runs between
             marching cubes and the export (one forward, one reverse and one albedo sweep per chunk inside the library, the
             vertices taken where marching cubes left them on the device) — with and without the one copy of its results
             to the host;
  loop       `validate_mesh_texture`'s loop (exp_runner.py:598-617) written with this package's direct calls: the host
             vertices of `extract_geometry` uploaded as float32, then per chunk of cut_size = 100000 vertices
             `sdf_network(vt)`, `sdf_network.gradient(vt)`, `color_network(vt, g, g, feat)` and the `.cpu()` of the albedo.

Model: the trained weights of the full_main_sharp fixture.  Milliseconds are wall-clock around a synchronised call (median
[min, max] of --reps after --warmup).  Also printed: V, and — not timed — the rms of the fp64 oracle's |sdf| over (a sample
of) the vertices with refine = 0 and refine = 2.

  python tools/textured_mesh_bench.py --res 512 --sparse --out profiles/textured_mesh_bench.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUT_SIZE = 100000


def _time(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
        del out
    return f"{statistics.median(ms):9.2f} [{min(ms):.2f}, {max(ms):.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--sparse", action="store_true", help="the SDF grid through extract_fields_sparse (the mesh is the same)")
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--oracle-sample", type=int, default=20000, help="vertices of the fp64 |sdf| figure (0: skip it)")
    ap.add_argument("--out", help="write the report here")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import rnb_neus_fork_amd as R
    from oracle import rnb_oracle as O
    from tests.golden_util import Golden

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    g = Golden("full_main_sharp")
    sdf_net, _, col_net, ren = R.build_from_named_params(g.mc, g.params(), dev)
    lo, hi = torch.tensor([-1.01] * 3), torch.tensor([1.01] * 3)
    res = a.res

    with torch.no_grad():
        if a.sparse:
            u, _ = ren.extract_fields_sparse(lo, hi, res, 0.0)
        else:
            u = ren.extract_fields(lo, hi, res, to_host=False)
        v_grid, tri = R.marching_cubes(u, 0.0)
        del u
    V = v_grid.shape[0]
    vertices = v_grid.cpu().numpy() / (res - 1.0) * (hi - lo).numpy()[None, :] + lo.numpy()[None, :]   # extract_geometry's

    def native_device():
        return ren.vertex_attributes(grid_vertices=v_grid, bounds=(lo, hi), resolution=res, chunk=a.chunk)

    def native_host():
        at = native_device()
        return {k: at[k].cpu().numpy() for k in ("normal", "rgb", "albedo", "sdf")}

    def loop():
        albedo = np.empty(vertices.shape)
        with torch.no_grad():
            chunks = torch.tensor(vertices).type(torch.float32).to(dev).split(CUT_SIZE)
            for k, vt in enumerate(chunks):
                out = sdf_net(vt)
                grad = sdf_net.gradient(vt).squeeze()
                alb = col_net(vt, grad, grad, out[:, 1:]).cpu().numpy()
                albedo[k * CUT_SIZE:k * CUT_SIZE + vt.shape[0]] = np.clip(alb[:, [2, 1, 0]], 0, 1)
        return albedo

    # the two stages compute the same colours (up to the routes' arithmetic: fused albedo sweep vs per-layer chain)
    nat, ref = native_host(), loop()
    diff = float(np.abs(nat["albedo"][:, [2, 1, 0]].clip(0, 1) - ref).max())
    t_dev = _time(native_device, a.reps, a.warmup)
    t_host = _time(native_host, a.reps, a.warmup)
    t_loop = _time(loop, a.reps, a.warmup)
    lines = [f"textured mesh, attribute stage; build {R.native.build_id()}; GPU: {torch.cuda.get_device_name(0)}",
             f"model full_main_sharp, box +-1.01, res {res}{' (sparse grid)' if a.sparse else ''}: V = {V} vertices, "
             f"T = {tri.shape[0]} triangles; chunk {a.chunk}; median [min, max] ms of {a.reps} calls after {a.warmup} warm-up",
             "",
             f"native vertex_attributes, results left on the device   {t_dev}",
             f"native vertex_attributes + one copy to the host        {t_host}",
             f"validate_mesh_texture's loop on the direct calls       {t_loop}",
             f"loop / native (+ host copy), medians                   "
             f"{float(t_loop.split()[0]) / float(t_host.split()[0]):9.2f}",
             f"max |clip(albedo) native - loop|                       {diff:9.2e}"]
    if a.oracle_sample > 0:
        torch.set_num_threads(16)
        p64 = {k: x.detach().double() for k, x in g.params().items()}
        pick = torch.randperm(V, generator=torch.Generator().manual_seed(0))[:a.oracle_sample]
        rms = {}
        for refine in (0, 2):
            at = ren.vertex_attributes(grid_vertices=v_grid, bounds=(lo, hi), resolution=res, refine=refine, chunk=a.chunk)
            x = at["points"].cpu()[pick].double()
            with torch.no_grad():
                rms[refine] = float(O.sdf_only(p64, g.mc.sdf, x).pow(2).mean().sqrt())
        lines += ["", f"rms of the fp64 oracle's |sdf| over {len(pick)} of the vertices: refine=0 {rms[0]:.3e}, "
                      f"refine=2 {rms[2]:.3e} (ratio {rms[0] / max(rms[2], 1e-300):.1f})"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
