"""The weight-gradient launch plan (csrc/dw_plan.h dw_make_plan) on the host, no GPU: tools/dw_plan_dump.hip is built host-only
and prints the plan dw_backward launches; it is held

  * to the launches of the commit before the planner existed, recorded by tools/gen_dw_plan_golden.py with that commit's
    dw.hip (tests/golden/dw_plan_parent.json: descriptors x variants x point counts x backward parts x sdf-head slabs), field
    for field, refusals included;
  * to the workspace sizes that commit's library answered, through the two workspace queries of the built library;
  * to the Python restatement of tests/point_matrix.py (plan_kind), for the bare job shapes and slab room it states;
  * to its own buffer: every partial slab inside [0, dw_part_floats), no two jobs of a launch overlapping, also when the
    workspace was carved for other parts than the backward asks for (then RNB_E_WORKSPACE, never an offset outside)."""
import functools
import json
import os
import shutil
import subprocess
import tempfile

import pytest

import rnb_neus_fork_amd as R
from tests import point_matrix as PM
from tools import gen_dw_plan_golden as GEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rnb-neus-fork_amd", "csrc")
J = {f: i for i, f in enumerate(["dW", "db", "N", "K", "lddw", "npairs", "bias_pair", "splits", "rows", "block_end", "part", "partb"])}


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "dw_plan_parent.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def dump_tool():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(tempfile.mkdtemp(prefix="dw_plan_dump_"), "dw_plan_dump")
    subprocess.run([hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-I", CSRC, "-I", os.path.join(ROOT, "tools"),
                    os.path.join(ROOT, "tools", "dw_plan_dump.hip"), os.path.join(CSRC, "layout.hip"), "-o", exe], check=True)
    return exe


def dump(lines):
    return [json.loads(t) for t in GEN.run(dump_tool(), lines)]


@functools.lru_cache(maxsize=None)
def recorded():
    """[(case, the plan the parent launched, the plan of this tree)] over the whole recorded matrix, one run of the tool"""
    g = golden()
    lines = [GEN.case_line(g["descriptors"][dn], g["variants"][vn], m, pn, slabs) for dn, vn, m, pn, slabs, _ in g["cases"]]
    assert g["parts"] == {pn: {"flags": list(f), "mode": mode} for pn, (f, mode) in GEN.PARTS.items()}
    return list(zip(g["cases"], [g["plans"][c[-1]] for c in g["cases"]], dump(lines)))


def test_the_recorded_matrix_is_the_one_asked_for():
    g = golden()
    cases = {tuple(c[:5]) for c in g["cases"]}
    assert len(cases) == len(g["cases"]) and cases == set(GEN.cases()) and g["parent"] == GEN.PARENT
    assert g["descriptors"] == GEN.descriptors() and g["variants"] == {v: R.native.variant_bits(**kw) for v, kw in GEN.VARIANTS.items()}
    # every descriptor on the default variant and every variant on the shipped shape meet the clamped row and a ragged one ...
    for dn in ("shipped", "sdf_nl12_albedo_nl4", "nl15", "albedo_w128", "mview0", "w100", "w288", "no_albedo_net"):
        assert {m for d, v, m, p, _ in cases if (d, v, p) == (dn, "default", "render(true,false)")} >= {1056, 726}
    for vn in GEN.VARIANTS:
        assert {m for d, v, m, p, _ in cases if (d, v, p) == ("shipped", vn, "render(true,false)")} >= {1056, 726}
        for dn in ("sdf_nl12_albedo_nl4", "albedo_w128", "w100", "w288"):      # (two groups; the split-K groups, exact and guarded)
            assert (dn, vn, 1056, "render(true,false)", 64) in cases
    # ... and the shipped shape on the default variant every point count with every part, with and without sdf-head slabs
    want_m = {r.M for r in PM.ROWS} | {726, 65536}
    for pn, (flags, _) in GEN.PARTS.items():
        assert {m for d, v, m, p, s in cases if (d, v, p) == ("shipped", "default", pn)} == want_m
        if flags[1]:
            assert {s for d, v, m, p, s in cases if (d, v, m, p) == ("shipped", "default", 1056, pn)} == {0, 64}
    # more one-workgroup jobs than a group holds make two groups; a refused combination is recorded as refused
    two = [p for c, p, _ in recorded() if c[:4] == ["sdf_nl12_albedo_nl4", "default", 1056, "render(true,false)"]]
    assert [[len(l["jobs"]) for l in p["launches"]] for p in two] == [[PM.K_MAX_DW_JOBS, 6]] * len(two) and two
    assert any("refused" in p for _, p, _ in recorded()) and any(p.get("slab_off", 0) > 0 for _, p, _ in recorded())


def test_planner_launches_what_the_parent_launched():
    bad = [(c[:5], want, got) for c, want, got in recorded() if want != got]
    assert not bad, f"{len(bad)} of {len(recorded())} recorded cases differ; the first: {bad[0]}"


def test_workspace_queries_answer_what_the_parent_answered():
    g, lib = golden(), R.native.load()
    queries = GEN.workspace_queries()
    assert len(queries) == len(g["workspace_bytes"])
    for q, want in zip(queries, g["workspace_bytes"]):
        got = GEN.workspace_answer(lib, g["descriptors"][q[0]], g["variants"][q[1]], *q[2:])
        assert got == want, f"{q}: {got} bytes, the parent answered {want}"


def _inside(plan):
    """every job's slabs lie in [0, floats) of dw_part, the one-workgroup kernel's behind slab_off; within a launch no overlap"""
    for l in plan["launches"]:
        spans = []
        for j in l["jobs"]:
            if j[J["part"]] < 0:
                assert j[J["partb"]] < 0 and l["nreduce"] == 0
                continue
            n = j[J["splits"]] * j[J["N"]]
            w = j[J["lddw"]] if l["block"] == 256 else j[J["K"]]      # (split-K slabs are [splits][N][lddw])
            assert j[J["partb"]] == j[J["part"]] + n * w
            spans.append((j[J["part"]], j[J["partb"]] + n))
            one_wg = l["block"] != 256
            lo, hi = (plan["slab_off"], plan["floats"]) if one_wg else (0, plan["slab_off"])
            assert lo <= spans[-1][0] and spans[-1][1] <= hi, (l["kernel"], j, plan["slab_off"], plan["floats"])
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (l["kernel"], spans)


def test_slabs_lie_inside_the_buffer_and_apart():
    for _, want, got in recorded():
        for plan in (want, got):
            if "refused" not in plan:
                _inside(plan)


@pytest.mark.parametrize("variant", ["default", "deterministic", "dw_staged+deterministic"])
def test_a_backward_the_workspace_was_not_carved_for_is_refused_or_fits(variant):
    """carved without the colour jobs (render_mode_of with NO_ALBEDO), launched with them, and the other way round: the boundary
    between the two parts of dw_part is the carving's, so the plan is held to it or refused with RNB_E_WORKSPACE"""
    g = golden()
    lines, names = [], []
    for m in (32, 726, 1056, 65536):
        for pn, mode in (("render(true,false)", 5), ("render(false,false)", 7), ("color_points(false)", 12), ("sdf_points(true,true)", 5)):
            flags = GEN.PARTS[pn][0]
            lines.append("D " + " ".join(str(x) for x in g["descriptors"]["shipped"] + [g["variants"][variant], m] + list(flags) + [mode, 0]))
            names.append((m, pn, mode))
    refused = 0
    for name, plan in zip(names, dump(lines)):
        if "refused" in plan:
            assert plan["refused"] == -2, (name, plan)      # RNB_E_WORKSPACE
            refused += 1
        else:
            _inside(plan)
    assert refused > 0 or variant == "default"


# ---------------------------------------------------------------------------------------------------------------------
# the restatement of tests/point_matrix.py
# ---------------------------------------------------------------------------------------------------------------------
def _job_line(m, jobs, room):
    """bare job shapes on the default route (x3, x2h, the one-workgroup kernel, no dw_lds, not deterministic); room < 0: unbounded"""
    return f"J {m} 1 1 1 0 0 0 0 {room} {len(jobs)} " + " ".join(f"{PM.N_ROWS} {w} {n}" for w, n in jobs)


@pytest.mark.parametrize("kind", sorted(PM.KINDS))
def test_restated_plan_is_the_planners(kind):
    k = PM.KINDS[kind]
    ms = [r.M for r in PM.X3_ROWS]
    held = dump([_job_line(m, k.jobs, PM.slab_room_floats(m, k)) for m in ms])
    free = dump([_job_line(m, k.jobs, -1) for m in ms])
    sized = dump([_job_line(m, k.sized, -1) for m in ms])
    for m, h, f, s in zip(ms, held, free, sized):
        assert s["slab_off"] == PM.slab_room_floats(m, k)          # (the tool prints the plan's two totals for a J line)
        (lh,), (lf,) = h["launches"], f["launches"]
        assert lh["kernel"] == "gemm_dw_x3_kernel<0, 2>" and lh["nreduce"] == len(k.jobs) and lh["grid"] == lh["jobs"][-1][J["block_end"]]
        got = [(j[J["K"]], j[J["npairs"]], j[J["splits"]], j[J["rows"]], m - (j[J["splits"]] - 1) * j[J["rows"]],
                j[J["splits"]] != u[J["splits"]]) for j, u in zip(lh["jobs"], lf["jobs"])]
        want = [(j.width, j.npairs, j.splits, j.rows, j.last_rows, j.clamped) for j in PM.plan_kind(m, kind)]
        assert got == want, f"{kind}, M = {m}"
        # the list's order reversed (most recent operands first): a bare job's dW is its index in the list
        assert [j[J["dW"]] for j in lh["jobs"]] == list(range(len(k.jobs) - 1, -1, -1))
        assert [j[J["block_end"]] for j in lh["jobs"]] == [sum(x[2] for x in want[:q + 1]) for q in range(len(want))]
