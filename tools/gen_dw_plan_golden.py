"""Recorded weight-gradient launch plans of the commit before the planner: tests/golden/dw_plan_parent.json.

TEST INFRASTRUCTURE ONLY, no GPU needed.  Checks the csrc of commit PARENT out of this repository's history into a scratch
directory, builds tools/dw_plan_parent_harness.hip against it (host only: that commit's dw.hip unmodified, its launch macro
replaced by a dump), runs it over the matrix below and writes inputs and launches down; tests/test_dw_plan_host.py holds
the planner of every later tree (csrc/dw_plan.h, through tools/dw_plan_dump.hip) to them.  Run it again only when a change
is MEANT to move a plan — and then against the commit before that change.

The workspace sizes that commit's LIBRARY answers (rnb_points_grad_workspace_bytes, rnb_render_workspace_bytes) are recorded
beside the plans when its build is given; without --parent-lib the section already in the file is kept.

    python tools/gen_dw_plan_golden.py [--parent-lib <checkout of PARENT, built>/rnb-neus-fork_amd/librnbneus_hip.so]
                                       [--out tests/golden/dw_plan_parent.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rnb_neus_fork_amd as R  # noqa: E402
from rnb_neus_fork_amd import runtime  # noqa: E402
from tests import point_matrix as PM  # noqa: E402
from tests import shape_matrix as SM  # noqa: E402

PARENT = "8adcc79"
DESC_FIELDS = ["sdf_d_in", "sdf_d_out", "sdf_d_hidden", "sdf_n_layers", "sdf_skip_in", "sdf_multires", "sdf_weight_norm",
               "col_d_feature", "col_d_in", "col_d_out", "col_d_hidden", "col_n_layers", "col_multires_view", "col_squeeze_out",
               "col_weight_norm", "n_samples", "n_importance", "up_sample_steps"]   # (then the variant bits)
K_SDF_HEAD_SLABS = 64   # rnb_internal.h kSdfHeadSlabs
PM_NORMAL, PM_COLOR, PM_BACKWARD, PM_NO_REVERSE = 1, 2, 4, 8   # rnb_internal.h PointMode

VARIANTS = {"default": dict(), "x2h=False": dict(x2h=False), "deterministic": dict(deterministic=True), "dw_lds": dict(dw_lds=True),
            "dw_staged": dict(dw_staged=True), "dw_staged+deterministic": dict(dw_staged=True, deterministic=True),
            "f32_mfma": dict(f32_mfma=True), "generic": dict(generic=True)}
# name -> (albedo, sdf, feat, normal, color_inputs) of BwdParts, the mode its API entry point carves the workspace with
# (api.hip render_mode_of / grad_mode)
_grad = lambda feat, normal, color=False: PM_BACKWARD | (PM_NORMAL if normal else PM_NO_REVERSE) | (PM_COLOR if feat or color else 0)
PARTS = {
    "render(true,false)": ((1, 1, 1, 1, 0), PM_NORMAL | PM_COLOR | PM_BACKWARD),
    "render(false,false)": ((0, 1, 0, 1, 0), PM_NORMAL | PM_BACKWARD),
    "render(true,true)": ((1, 1, 1, 1, 1), PM_NORMAL | PM_COLOR | PM_BACKWARD),
    "sdf_points(false,false)": ((0, 1, 0, 0, 0), _grad(False, False)),
    "sdf_points(true,false)": ((0, 1, 1, 0, 0), _grad(True, False)),
    "sdf_points(false,true)": ((0, 1, 0, 1, 0), _grad(False, True)),
    "sdf_points(true,true)": ((0, 1, 1, 1, 0), _grad(True, True)),
    "color_points(false)": ((1, 0, 0, 0, 0), _grad(False, False, True)),
    "color_points(true)": ((1, 0, 0, 0, 1), _grad(False, False, True)),
}
ALL_M = [r.M for r in PM.X3_ROWS] + [r.M for r in PM.RAGGED_ROWS] + [726, 65536]
SHORT_M = [32, 1056, 726, 65536]     # one split per job; a clamped row; a ragged render step; the bench's size


def _ints(d):
    return [int(getattr(d, f)) for f in DESC_FIELDS]


def descriptors():
    by_name = {s.name: s for s in SM.SHAPES}
    mc = lambda **kw: SM._mc(render=SM.WIDE_RENDER, **kw)
    sdf = R.SDFNetwork(d_in=3, d_out=257, d_hidden=256, n_layers=8, skip_in=[4], multires=6)
    col = R.RenderingNetwork(d_feature=256, mode="no_view_dir", d_in=6, d_out=3, d_hidden=256, n_layers=2, multires_view=4)
    out = {"shipped": _ints(R.model_desc(sdf, col)),
           "sdf_nl12_albedo_nl4": _ints(SM.desc_of(mc(n_layers=12, color=dict(n_layers=4))))}    # 17 one-workgroup jobs: two groups
    for name in ("nl15", "albedo_w128", "mview0", "w100", "w288"):
        out[name] = _ints(SM.desc_of(by_name[name].mc))
    out["no_albedo_net"] = _ints(R.model_desc(sdf, None))          # the direct SDFNetwork calls: a 32-wide placeholder albedo net
    out["albedo_net_alone"] = _ints(runtime._color_desc(col, 256, 6))   # the direct RenderingNetwork calls
    # no feature head, no albedo net: the library refuses the colour and feature parts
    out["no_feature_head"] = _ints(R.model_desc(R.SDFNetwork(d_in=3, d_out=1, d_hidden=256, n_layers=8, skip_in=[4], multires=6), None))
    return out


def cases():
    """(descriptor, variant, M, parts, sdfh_slabs).  The shipped shape on the default variant meets every point count with every
    part; each other descriptor and each other variant meets the clamped row and a ragged one; the rest of the cross product is
    thinned (the file is read by people too).  sdfh_slabs is what the backward passes (kSdfHeadSlabs when the one-workgroup
    kernel's reduction can take the sdf-head row, else 0); both values at M = 1056 and 726 of the shipped shape."""
    natural = lambda m, flags: K_SDF_HEAD_SLABS if flags[1] and m % 32 == 0 else 0
    some = ("render(true,false)", "render(false,false)", "sdf_points(true,false)", "color_points(false)")
    out = []
    for dn in descriptors():
        for vn in VARIANTS:
            if dn == "shipped" and vn == "default":
                picks = [(m, pn) for m in ALL_M for pn in PARTS]
            elif dn == "no_feature_head":
                picks = [(1056, pn) for pn in PARTS] if vn == "default" else []
            elif vn == "default":
                picks = [(m, pn) for m in (1056, 726) for pn in some if pn != "sdf_points(true,false)"]
            elif dn == "shipped":
                picks = [(m, pn) for m in (1056, 726) for pn in some] + [(65536, "render(true,false)")]
            else:
                picks = [(1056, "render(true,false)")] if dn in ("sdf_nl12_albedo_nl4", "albedo_w128", "w100", "w288") else []
            for m, pn in picks:
                flags = PARTS[pn][0]
                both = dn == "shipped" and vn == "default" and m in (1056, 726) and flags[1]
                for slabs in ((0, K_SDF_HEAD_SLABS) if both else (natural(m, flags),)):
                    out.append((dn, vn, m, pn, slabs))
    return out


def case_line(desc_ints, variant_bits, m, parts_name, slabs):
    flags, mode = PARTS[parts_name]
    return "D " + " ".join(str(x) for x in list(desc_ints) + [variant_bits, m] + list(flags) + [mode, slabs])


def run(tool, lines):
    r = subprocess.run([tool], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    out = r.stdout.splitlines()
    assert len(out) == len(lines), (len(out), len(lines))
    return out


def build_parent_harness(tmp):
    src = os.path.join(tmp, "parent")
    os.makedirs(src)
    tar = subprocess.run(["git", "-C", ROOT, "archive", PARENT, "rnb-neus-fork_amd/csrc", "include"], capture_output=True, check=True)
    subprocess.run(["tar", "-x", "-C", src], input=tar.stdout, check=True)
    csrc = os.path.join(src, "rnb-neus-fork_amd", "csrc")
    exe = os.path.join(tmp, "dw_plan_parent_harness")
    subprocess.run(["hipcc", "--cuda-host-only", "-std=c++17", "-O1", "-I", csrc, "-I", os.path.join(ROOT, "tools"),
                    os.path.join(ROOT, "tools", "dw_plan_parent_harness.hip"), os.path.join(csrc, "layout.hip"), "-o", exe], check=True)
    return exe


POINT_FLAGS = {"FEATURE": 1, "NORMAL": 2, "FEATURE|NORMAL": 3, "COLOR": 4}          # rnbneus.h RNB_POINTS_*
RENDER_SHAPES = [(33, 22), (3, 352), (512, 128)]                                     # (B, S): M = 726, 1056, 65536


def workspace_queries():
    """[(descriptor, variant, "points" | "render", a, b, flags)]: n points, flags | B, S, flags"""
    N = R.native
    out = []
    for dn in ("shipped", "no_albedo_net", "albedo_net_alone", "w288"):
        for vn in VARIANTS:
            out += [(dn, vn, "points", m, 0, f) for m in SHORT_M for f in POINT_FLAGS.values()]
            out += [(dn, vn, "render", b, s, f) for b, s in RENDER_SHAPES for f in (N.MODE_MVPS, N.MODE_MVPS | N.FLAG_NO_ALBEDO)]
    return out


def workspace_answer(lib, desc_ints, variant_bits, kind, a, b, flags):
    """the library's answer: bytes, or its (negative) error code"""
    d = R.native.ModelDesc()
    for f, v in zip(DESC_FIELDS, desc_ints):
        setattr(d, f, v)
    d.sdf_scale, d.variant = 1.0, variant_bits
    n = C.c_int64(-1)
    if kind == "points":
        rc = lib.rnb_points_grad_workspace_bytes(C.byref(d), C.c_int64(a), C.c_int32(flags), C.byref(n))
    else:
        rc = lib.rnb_render_workspace_bytes(C.byref(d), C.c_int64(a), C.c_int32(b), C.c_int32(flags), C.byref(n))
    return n.value if rc == 0 else rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "dw_plan_parent.json"))
    args = ap.parse_args()
    descs = descriptors()
    bits = {vn: R.native.variant_bits(**kw) for vn, kw in VARIANTS.items()}
    cs = cases()
    with tempfile.TemporaryDirectory() as tmp:
        got = run(build_parent_harness(tmp), [case_line(descs[dn], bits[vn], m, pn, slabs) for dn, vn, m, pn, slabs in cs])
    plans, index = [], {}
    rows = []
    for c, text in zip(cs, got):
        if text not in index:
            index[text] = len(plans)
            plans.append(json.loads(text))
        rows.append(list(c) + [index[text]])
    out = {"parent": PARENT, "desc_fields": DESC_FIELDS, "descriptors": descs, "variants": bits,
           "parts": {pn: {"flags": list(f), "mode": mode} for pn, (f, mode) in PARTS.items()},
           "job_fields": ["dW", "db", "N", "K", "lddw", "npairs", "bias_pair", "splits", "rows_per_split", "block_end", "part", "partb"],
           "extra_fields": ["dW", "db", "N", "K", "lddw", "splits", "block_end", "sdfh_part", "partb-part"],
           "case_fields": ["descriptor", "variant", "M", "parts", "sdfh_slabs", "plan"], "cases": rows, "plans": plans}
    if args.parent_lib:
        lib = C.CDLL(args.parent_lib)
        out["workspace_bytes"] = [workspace_answer(lib, descs[q[0]], bits[q[1]], *q[2:]) for q in workspace_queries()]
    else:
        out["workspace_bytes"] = json.load(open(args.out))["workspace_bytes"]
    js = lambda x: json.dumps(x, separators=(",", ":"))
    with open(args.out, "w") as f:     # (one plan per line, the cases of one descriptor and variant per line)
        f.write("{" + ",\n".join(f"{js(k)}:{js(v)}" for k, v in out.items() if k not in ("cases", "plans")))
        groups = {}
        for r in rows:
            groups.setdefault((r[0], r[1]), []).append(r)
        f.write(',\n"cases":[\n' + ",\n".join(js(grp)[1:-1] for grp in groups.values()) + "\n]")
        f.write(',\n"plans":[\n' + ",\n".join(js(p) for p in plans) + "\n]}\n")
    refused = sum("refused" in plans[r[-1]] for r in rows)
    print(f"{len(rows)} cases ({refused} refused), {len(plans)} distinct plans from commit {PARENT} -> {args.out} "
          f"({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
