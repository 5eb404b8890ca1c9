"""Times the opt-in autograd of the direct network calls against torch autograd through the fp32 oracle on the same GPU.

Case "eikonal": ((sdf_network.gradient(x).norm(-1) - 1)^2).mean(), forward + backward into every SDF leaf.
Case "texture": Runner.validate_mesh_texture's three calls (sdf_hidden_appearance, gradient, color_network) and a loss on
the albedo, forward + backward into every leaf of both networks.
Both outputs are checked against each other first.  Device events, warm-up, median of --reps.  Prints one JSON line per
(case, n, impl) and a markdown table.

  python tools/field_autograd_bench.py [--n 65536 100000] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rnb_neus_fork_amd as R  # noqa: E402
from oracle import rnb_oracle as O  # noqa: E402


def _time(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    fw, bw = [], []
    for _ in range(reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        loss = fn(backward=False)
        e[1].record()
        loss.backward()
        e[2].record()
        torch.cuda.synchronize()
        fw.append(e[0].elapsed_time(e[1]))
        bw.append(e[1].elapsed_time(e[2]))
    return statistics.median(fw), statistics.median(bw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 100000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    mc = O.ModelConf()
    torch.manual_seed(0)
    p = O.init_params(mc)
    sdf, _, col, _ = R.build_from_named_params(mc, p, dev)
    sdf.set_autograd(True)
    col.set_autograd(True)
    q = {k: v.to(dev).requires_grad_(k.startswith(("sdf.", "color."))) for k, v in p.items()}
    rows = []
    for n in a.n:
        g = torch.Generator().manual_seed(n)
        x = (torch.rand(n, 3, generator=g) * 1.8 - 0.9).to(dev)
        Wa = torch.randn(n, 3, generator=g).to(dev)

        def oracle_normal(v):
            v = v.detach().requires_grad_(True)
            y = O.sdf_only(q, mc.sdf, v)
            return torch.autograd.grad(y, v, torch.ones_like(y), create_graph=True)[0]

        cases = {
            "eikonal": (lambda backward=True: ((sdf.gradient(x).norm(dim=-1) - 1) ** 2).mean(),
                        lambda backward=True: ((oracle_normal(x).norm(dim=-1) - 1) ** 2).mean()),
            "texture": (lambda backward=True: (Wa * col(x, *(2 * [sdf.gradient(x).squeeze(1)]),
                                                          sdf.sdf_hidden_appearance(x)[:, 1:])).sum(),
                        lambda backward=True: (Wa * (lambda nr: O.color_forward(q, mc.color, x, nr, nr,
                                                                                O.sdf_forward(q, mc.sdf, x)[:, 1:]))(
                                                    oracle_normal(x))).sum()),
        }
        for case, (mine, ref) in cases.items():
            lm, lr = float(mine().detach()), float(ref().detach())
            rel = abs(lm - lr) / max(abs(lr), 1e-30)
            assert rel < 1e-3, f"{case} n={n}: native loss {lm} vs torch fp32 {lr}"
            for impl, fn in (("native", mine), ("torch_fp32", ref)):
                f, b = _time(fn, a.reps, a.warmup)
                row = dict(case=case, n=n, impl=impl, fwd_ms=round(f, 3), bwd_ms=round(b, 3), total_ms=round(f + b, 3),
                           loss_rel_diff=rel, build_id=R.native.build_id())
                rows.append(row)
                print(json.dumps(row), flush=True)
    print("\n| case | n | impl | forward ms | backward ms | total ms |\n|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['case']} | {r['n']} | {r['impl']} | {r['fwd_ms']} | {r['bwd_ms']} | {r['total_ms']} |")


if __name__ == "__main__":
    main()
