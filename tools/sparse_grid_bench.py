"""Times `NeuSRenderer.extract_fields_sparse` against the dense `extract_fields(to_host=False)` on one GPU.

Models: the seed-0 geometric init of the full-size network ("geo") and the trained weights of the full_main_sharp fixture
("sharp").  For every resolution, brick size and margin: milliseconds of the whole call (device events around it, so the
per-round 8-byte read-backs and the gaps they leave are inside; median, min and max of --reps after --warmup), bricks seeded /
active / total, growth rounds, points evaluated.  Next to it the dense grid at the same resolution (`extract_fields` while its
single launch fits the runtime's limit of 2^32 threads, i.e. below 2^30 points; beyond, the same `rnb_sdf_grid` called per
x-slab of at most 2^29 points into one volume: "slabs"), on this build and — with
--baseline FILE, the JSON a `--dense-only --json FILE` run of this tool wrote for another build (`--tree DIR` imports the
package from there) — on that build.

  python tools/sparse_grid_bench.py --tree ../parent --dense-only --json dense_parent.json
  python tools/sparse_grid_bench.py --baseline dense_parent.json --out profiles/sparse_grid.txt
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _time(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
        del out
    return {"ms": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def _dense(R, ren, lo, hi, res):
    """the dense volume on the device: extract_fields, or rnb_sdf_grid per x-slab where one launch would be too large"""
    import ctypes as C
    if res ** 3 < 2 ** 30:
        return ren.extract_fields(lo, hi, res, to_host=False)
    lib, native = R.native.load(), R.native
    dev = ren.sdf_network.lin0.bias.device
    planes = max(1, 2 ** 29 // (res * res))
    with torch.no_grad():
        packed = ren._pack(False)
        u = torch.empty(res, res, res, dtype=torch.float32, device=dev)
        gd = native.GridDesc()
        for d in range(3):
            gd.bound_min[d], gd.bound_max[d] = float(lo[d]), float(hi[d])
        gd.resolution, gd.out_scale = res, -1.0
        ws = None
        for x0 in range(0, res, planes):
            gd.x_begin, gd.x_end = x0, min(x0 + planes, res)
            if ws is None:
                nbytes = C.c_int64()
                native.check(lib.rnb_sdf_grid_workspace_bytes(C.byref(ren.desc), C.byref(gd), C.byref(nbytes)))
                ws = torch.empty(max(nbytes.value, 256), dtype=torch.uint8, device=dev)
            with native.on_device(dev) as stream:
                native.check(lib.rnb_sdf_grid(C.byref(ren.desc), native.ptr(packed), C.byref(gd), native.ptr(u[x0:]),
                                              native.ptr(ws), ws.numel(), stream))
    return u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[512, 1024, 1536])
    ap.add_argument("--bricks", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--margins", type=float, nargs="+", default=[0.0, 1.0])
    ap.add_argument("--models", nargs="+", default=["geo", "sharp"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tree", default=ROOT, help="import rnb_neus_fork_amd from this checkout")
    ap.add_argument("--dense-only", action="store_true")
    ap.add_argument("--json", help="write the rows here")
    ap.add_argument("--baseline", help="JSON of a --dense-only run on the build to compare against")
    ap.add_argument("--out", help="write the table here")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(1, ROOT)
    import rnb_neus_fork_amd as R
    from oracle import rnb_oracle as O
    from tests.golden_util import Golden

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    build = R.native.build_id()
    lo, hi = torch.tensor([-1.01] * 3), torch.tensor([1.01] * 3)
    rows = []
    for which in a.models:
        if which == "geo":
            mc = O.ModelConf()
            torch.manual_seed(0)
            p = O.init_params(mc)
        else:
            g = Golden("full_main_sharp")
            mc, p = g.mc, g.params()
        ren = R.build_from_named_params(mc, p, dev)[3]
        for res in a.res:
            row = dict(kind="dense", model=which, res=res, build_id=build, how="one call" if res ** 3 < 2 ** 30 else "slabs",
                       **_time(lambda: _dense(R, ren, lo, hi, res), a.reps, a.warmup))
            rows.append(row)
            print(json.dumps(row), flush=True)
            if a.dense_only:
                continue
            for bs in a.bricks:
                for margin in a.margins:
                    info = {}

                    def run():
                        u, i = ren.extract_fields_sparse(lo, hi, res, brick=bs, margin=margin)
                        info.update(i)
                        return u
                    t = _time(run, a.reps, a.warmup)
                    row = dict(kind="sparse", model=which, res=res, brick=bs, margin=margin, build_id=build, **t,
                               seeded=info["bricks_seeded"], active=info["bricks_active"], total=info["bricks_total"],
                               rounds=info["rounds"], points=info["points_evaluated"])
                    rows.append(row)
                    print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f)
    base = {}
    if a.baseline:
        for r in json.load(open(a.baseline)):
            base[(r["model"], r["res"])] = r
    dense = {(r["model"], r["res"]): r for r in rows if r["kind"] == "dense"}
    lines = [f"sparse SDF grid vs dense extract_fields(to_host=False); build {build}; "
             f"median [min, max] ms of {a.reps} calls after {a.warmup} warm-up, device events around the whole call",
             f"GPU: {torch.cuda.get_device_name(0)}; box +-1.01", ""]
    if base:
        lines.append(f"dense baseline build: {next(iter(base.values()))['build_id']}")
    lines.append("model  res   how      dense ms (this build)        dense ms (baseline build)")
    for k, r in dense.items():
        b = base.get(k)
        lines.append(f"{k[0]:6s} {k[1]:5d} {r['how']:8s} {r['ms']:9.2f} [{r['min']:.2f}, {r['max']:.2f}]"
                     + (f"   {b['ms']:9.2f} [{b['min']:.2f}, {b['max']:.2f}]" if b else "   not measured"))
    lines += ["", "model  res   brick margin   sparse ms [min, max]          seeded   active    total  active%  rounds"
              "       points  pts/dense%  dense/sparse"]
    for r in rows:
        if r["kind"] != "sparse":
            continue
        d = base.get((r["model"], r["res"]), dense[(r["model"], r["res"])])
        lines.append(f"{r['model']:6s} {r['res']:5d} {r['brick']:5d} {r['margin']:6.1f} {r['ms']:9.2f} [{r['min']:.2f}, {r['max']:.2f}]"
                     f" {r['seeded']:9d} {r['active']:8d} {r['total']:8d} {100 * r['active'] / r['total']:7.2f} {r['rounds']:7d}"
                     f" {r['points']:12d} {100 * r['points'] / r['res'] ** 3:10.2f} {d['ms'] / r['ms']:12.2f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
