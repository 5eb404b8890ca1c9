"""Recorded workspace sizes of the bf16 route: tests/golden/bf16_workspace_parent.json.

TEST INFRASTRUCTURE ONLY, no GPU needed.  Asks the built library of the tree this script is run FROM for
`rnb_render_workspace_bytes` over the matrix of tests/test_bf16_plan_host.py and writes the answers down.  It was run in a
checkout of the commit before the bf16 unit was split and its weight-gradient plan gathered into one function (copy this
file there, build, run it with `--out`); the test holds every later tree to those numbers.  Run it again only when a
change is MEANT to move a bf16 workspace size.

    python tools/gen_bf16_workspace_golden.py [--out tests/golden/bf16_workspace_parent.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rnb_neus_fork_amd as R  # noqa: E402

N = R.native

# name -> (SDF d_out, albedo hidden layers, multires_view)
SHAPES = {
    "shipped": (257, 2, 4),          # bf16 albedo kernels
    "feature255": (256, 2, 4),       # feature width 255: fp32 albedo kernels behind the bf16 SDF sweeps
    "albedo3_mv4": (257, 3, 4),      # three hidden albedo layers, still the bf16 albedo kernels
}
VARIANTS = {"bf16": N.VARIANT_BF16, "bf16+deterministic": N.VARIANT_BF16 | N.VARIANT_DETERMINISTIC}
BS = (1, 37, 512)
SS = (128, 256)
FLAGS = {"mvps": N.MODE_MVPS, "mvps|no_albedo": N.MODE_MVPS | N.FLAG_NO_ALBEDO,
         "mvps|forward_only": N.MODE_MVPS | N.FLAG_FORWARD_ONLY}


def desc(shape, variant):
    d_out, n_layers, multires_view = SHAPES[shape]
    sdf = R.SDFNetwork(d_in=3, d_out=d_out, d_hidden=256, n_layers=8, skip_in=[4], multires=6)
    col = R.RenderingNetwork(d_feature=d_out - 1, mode="no_view_dir", d_in=6, d_out=3, d_hidden=256, n_layers=n_layers,
                             multires_view=multires_view)
    d = R.model_desc(sdf, col)
    d.variant = VARIANTS[variant]
    return d


def key(variant, shape, B, S, flags):
    return f"{variant} {shape} B={B} S={S} {flags}"


def cases():
    return [(v, sh, B, S, f) for v in VARIANTS for sh in SHAPES for B in BS for S in SS for f in FLAGS]


def workspace_bytes(d, B, S, flags):
    b = C.c_int64()
    N.check(N.load().rnb_render_workspace_bytes(C.byref(d), B, S, flags, C.byref(b)))
    return b.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "bf16_workspace_parent.json"))
    args = ap.parse_args()
    descs = {(v, sh): desc(sh, v) for v in VARIANTS for sh in SHAPES}
    out = {"build_id": N.load().rnb_build_id().decode(), "abi_version": int(N.load().rnb_abi_version()),
           "bytes": {key(*c): workspace_bytes(descs[c[0], c[1]], c[2], c[3], FLAGS[c[4]]) for c in cases()}}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"{len(out['bytes'])} sizes from build {out['build_id']} -> {args.out}")


if __name__ == "__main__":
    main()
