"""Times the cleanup of a marching-cubes mesh with floaters — keep the largest connected component — three ways:

  (a) device   `clean_mesh(v, t, keep_largest=1)` on the tensors marching cubes left on the GPU (csrc/mesh_clean.hip), results
               left on the device, and with the one copy of the cleaned mesh to the host;
  (b) host     what a user does without it: copy V x 3 doubles and T x 3 ints to the host,
               `scipy.sparse.csgraph.connected_components` over the triangle edges (when scipy imports; else said so),
               triangle areas per component with numpy, numpy compaction;
  (c) model    `extract_textured_geometry` of the full_main_sharp fixture with and without `clean={"keep_largest": 1}`
               (--model-res; 0 skips it).

Mesh of (a) and (b): the native marching cubes at --res of an analytic volume on [-1, 1]^3 — a sphere of radius 0.55 and
--floaters small spheres (radius 0.02 .. 0.06, seeded) around it.  Milliseconds are wall-clock around a synchronised call:
median [min, max] over --reps blocks of calls (--inner per block for the device route), after --warmup blocks.

  python tools/mesh_clean_bench.py --res 512 --out profiles/mesh_clean_bench.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _time(fn, reps, warmup, inner):
    """per-call milliseconds: (median, min, max) over `reps` blocks of `inner` calls"""
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


def _fmt(t):
    return f"{t[0]:10.2f} [{t[1]:.2f}, {t[2]:.2f}]"


def floater_volume(res, n_floaters, dev, seed=0):
    """u = -sdf of the union of a sphere of radius 0.55 and n small spheres, [res]^3 fp32 on the device, built slab by slab"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n_floaters, 3))
    centres = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.7, 0.9, (n_floaters, 1))
    radii = rng.uniform(0.02, 0.06, n_floaters)
    spheres = [((0.0, 0.0, 0.0), 0.55)] + [(tuple(c), float(r)) for c, r in zip(centres, radii)]
    ax = torch.linspace(-1.0, 1.0, res, device=dev)
    u = torch.empty(res, res, res, device=dev)
    step = max(1, (1 << 24) // (res * res))
    for x0 in range(0, res, step):
        x = ax[x0:x0 + step, None, None]
        best = torch.full((x.shape[0], res, res), -1e9, device=dev)
        for c, r in spheres:
            dist = torch.sqrt((x - c[0]) ** 2 + (ax[None, :, None] - c[1]) ** 2 + (ax[None, None, :] - c[2]) ** 2)
            best = torch.maximum(best, r - dist)
        u[x0:x0 + step] = best
    return u


def host_route(v_dev, t_dev, csgraph):
    """the detour a user takes today: the mesh to the host, a host graph library, numpy compaction"""
    import scipy.sparse as sp
    v, t = v_dev.cpu().numpy(), t_dev.cpu().numpy()
    V = len(v)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]]])
    g = sp.coo_matrix((np.ones(len(e), dtype=np.int8), (e[:, 0], e[:, 1])), shape=(V, V))
    n, lab = csgraph.connected_components(g, directed=False)
    p = v[t]
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    tl = lab[t[:, 0]]
    best = int(np.argmax(np.bincount(tl, weights=area, minlength=n)))
    keep_v = lab == best
    newidx = np.cumsum(keep_v) - 1
    return v[keep_v], newidx[t[tl == best]].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--floaters", type=int, default=200)
    ap.add_argument("--model-res", type=int, default=256, help="resolution of the extract_textured_geometry timing (0: skip)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", help="write the report here")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import rnb_neus_fork_amd as R

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    u = floater_volume(a.res, a.floaters, dev)
    v, t = R.marching_cubes(u, 0.0)
    del u
    comp = R.mesh_components(t, vertices=v)

    def device_clean():
        return R.clean_mesh(v, t, keep_largest=1)

    def device_clean_to_host():
        out = device_clean()
        return out["vertices"].cpu().numpy(), out["triangles"].cpu().numpy()

    def components_only():
        return R.mesh_components(t, vertices=v)

    lines = [f"mesh cleanup, keep the largest component; build {R.native.build_id()}; GPU: {torch.cuda.get_device_name(0)}",
             f"analytic volume at res {a.res}: a sphere + {a.floaters} small spheres; V = {len(v)} vertices, T = {len(t)} "
             f"triangles, C = {comp['n_components']} components",
             f"per-call ms, median [min, max] over {a.reps} blocks after {a.warmup} warm-up blocks; calls per block: (a) {a.inner}, "
             f"(b) 1, (c) 5", ""]
    cv, ct = device_clean_to_host()
    lines.append(f"kept: V' = {len(cv)}, T' = {len(ct)}")
    t_comp = _time(components_only, a.reps, a.warmup, a.inner)
    t_dev = _time(device_clean, a.reps, a.warmup, a.inner)
    t_dev_host = _time(device_clean_to_host, a.reps, a.warmup, a.inner)
    lines += [f"(a) mesh_components alone (labels + statistics)         {_fmt(t_comp)}",
              f"(a) clean_mesh, results left on the device              {_fmt(t_dev)}",
              f"(a) clean_mesh + one copy of the cleaned mesh to host   {_fmt(t_dev_host)}"]
    try:
        from scipy.sparse import csgraph
    except ImportError:
        csgraph = None
        lines.append("(b) host route: scipy is not importable here: not measured")
    if csgraph is not None:
        hv, ht = host_route(v, t, csgraph)
        same = np.array_equal(hv, cv) and np.array_equal(ht, ct)
        t_host = _time(lambda: host_route(v, t, csgraph), a.reps, a.warmup, 1)
        lines += [f"(b) host route: copy to host, scipy components, numpy    {_fmt(t_host)}",
                  f"    host / device (+ host copy), medians                 {t_host[0] / t_dev_host[0]:10.2f}",
                  f"    the two routes give the same arrays: {same}"]
    if a.model_res > 0:
        from tests.golden_util import Golden
        g = Golden("full_main_sharp")
        ren = R.build_from_named_params(g.mc, g.params(), dev)[3]
        lo, hi = torch.tensor([-1.01] * 3), torch.tensor([1.01] * 3)
        plain = ren.extract_textured_geometry(lo, hi, a.model_res, sparse=True)
        cleaned = ren.extract_textured_geometry(lo, hi, a.model_res, sparse=True, clean={"keep_largest": 1})
        info = ren.last_mesh_clean
        t_plain = _time(lambda: ren.extract_textured_geometry(lo, hi, a.model_res, sparse=True), a.reps, a.warmup, 5)
        t_clean = _time(lambda: ren.extract_textured_geometry(lo, hi, a.model_res, sparse=True, clean={"keep_largest": 1}),
                        a.reps, a.warmup, 5)
        lines += ["", f"(c) full_main_sharp, extract_textured_geometry(sparse=True) at res {a.model_res}: "
                      f"{info['n_components']} components, V = {len(plain['vertices'])} -> {len(cleaned['vertices'])}",
                  f"    clean=None                                           {_fmt(t_plain)}",
                  f"    clean={{'keep_largest': 1}}                             {_fmt(t_clean)}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
