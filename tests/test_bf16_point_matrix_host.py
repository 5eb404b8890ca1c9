"""tests/bf16_point_matrix.py on the host, no GPU: the table meets every class it claims; its restatement of the bf16 route's
weight-gradient split plan equals the library's (csrc/bf16_dw_plan.h, printed by tools/dw_plan_dump.hip built host-only, and
the deterministic variant's slab bytes in `rnb_render_workspace_bytes`); every row is accepted by the workspace queries; and
the tail recipe of the device test (tests/test_gpu_bf16_point_matrix.py, part B) puts at least half of the last ray's
`weights` on the points of the last K8 unit, in the fp64 oracle."""
import ctypes as C
import functools
import json
import os
import shutil
import subprocess
import tempfile

import pytest

import rnb_neus_fork_amd as R
from tests import bf16_point_matrix as BM
from tests.golden_util import Golden
from tests.shape_matrix import desc_of
from tools import gen_dw_plan_golden as GEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rnb-neus-fork_amd", "csrc")
SDF_BF16, COLOR_LAYERS, COLOR_BF16 = 2, 1, 3        # rnb_internal.h SdfRoute / ColorRoute


def _desc(row, **variant):
    d = desc_of(row.model_conf, bf16=True, **variant)
    rc = row.render
    d.n_samples, d.n_importance, d.up_sample_steps = rc.n_samples, rc.n_importance, rc.up_sample_steps
    return d


@functools.lru_cache(maxsize=None)
def dump_tool():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(tempfile.mkdtemp(prefix="dw_plan_dump_"), "dw_plan_dump")
    subprocess.run([hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-I", CSRC, "-I", os.path.join(ROOT, "tools"),
                    os.path.join(ROOT, "tools", "dw_plan_dump.hip"), os.path.join(CSRC, "layout.hip"), "-o", exe], check=True)
    return exe


def library_plan(row):
    """the library's plan of the row's descriptor, point count and with_color"""
    d = _desc(row)
    line = "B " + " ".join(str(x) for x in GEN._ints(d) + [int(d.variant), row.M, 0 if row.no_albedo else 1])
    return json.loads(GEN.run(dump_tool(), [line])[0])


# ------------------------------------------------------------------------------------------------------------- the table
def test_the_rows_are_the_ones_asked_for():
    assert [(r.B, r.S, r.M) for r in BM.ROWS[:6]] == [(1, 22, 22), (3, 22, 66), (3, 25, 75), (172, 16, 2752), (126, 22, 2772),
                                                      (502, 11, 5522)]
    assert [r.name for r in BM.ROWS[6:]] == ["3x22_no_albedo", "3x22_render", "3x25_mv6"]
    assert all(r.M <= 6000 and r.why for r in BM.ROWS)
    for names in (BM.DETERMINISTIC_ROWS, BM.TAIL_ROWS, BM.POISON_ROWS):
        assert all(n in BM.BY_NAME for n in names)
    assert [BM.BY_NAME[n].M for n in BM.DETERMINISTIC_ROWS] == [22, 75, 2772, 5522]
    assert [BM.BY_NAME[n].M for n in BM.TAIL_ROWS] == [66, 75, 2772, 5522]
    assert [BM.BY_NAME[n].tail for n in BM.TAIL_ROWS] == [2, 3, 4, 2]
    assert [BM.BY_NAME[n].M for n in BM.POISON_ROWS] == [75, 2772]


def test_every_class_is_met_by_some_row():
    plans = [r.plan for r in BM.ROWS]
    assert {r.jobs_name: r.plan.njobs for r in BM.ROWS} == {"shipped": 12, "no_albedo": 8, "fp32_albedo": 9}
    assert {BM.tail_class(r.M) for r in BM.ROWS} >= {"0", "1..7", "9..15"}
    # an odd M: the last bf16 PAIR of a unit holds one point and one padded row (the two constants of bf_dw_mask_tail)
    assert any(r.M % 2 == 1 for r in BM.ROWS) and any(r.M % 2 == 1 for r in map(BM.BY_NAME.get, BM.TAIL_ROWS + BM.POISON_ROWS))
    assert {p.last_chunks for p in plans} >= {1, 2, 3, 5}
    assert {p.full_chunks for p in plans} >= {2, 4, 6}
    assert {p.last_steps % 3 for p in plans} == {0, 1, 2}
    assert {p.splits for p in plans} >= {1, 2}                       # a launch of one split, and one with a short last split
    assert any(p.last_rows == p.rows and p.splits > 1 for p in plans)     # ... and one whose last split is full
    assert any(p.last_rows % BM.K_CHUNK for p in plans if p.last_chunks >= 3)          # a ragged last chunk behind whole ones
    # a padded row exists in every row, up to half a pad and beyond
    assert all(r.Mp > r.M for r in BM.ROWS) and {r.Mp - r.M for r in BM.ROWS} >= {64, 106, 62, 53, 44, 110}
    # the head-backward kernels: several blocks with a ragged last one, and the deterministic variant's single block
    assert {BM.rows_per_slab(r.M, False) for r in BM.ROWS} >= {(3, 8), (9, 8), (10, 8), (172, 16), (174, 16), (231, 24)}
    assert all(BM.rows_per_slab(r.M, True)[0] == 1 and BM.rows_per_slab(r.M, True)[1] >= r.M for r in BM.ROWS)
    # the rows as the issue names them
    by = BM.BY_NAME
    assert (by["1x22"].plan.splits, by["1x22"].plan.last_chunks, by["1x22"].M % 16) == (1, 1, 6)
    assert (by["3x22"].plan.splits, by["3x22"].plan.full_chunks, by["3x22"].plan.last_rows) == (2, 2, 2)
    assert (by["3x25"].plan.last_rows, by["3x25"].M % 16) == (11, 11)
    assert (by["172x16"].plan.splits, by["172x16"].plan.rows, by["172x16"].plan.last_rows) == (43, 64, 64)
    assert BM.dw_plan(2753, BM.JOBS["shipped"]).rows == 128         # "the last M before rows per split becomes 128"
    assert (by["126x22"].plan.rows, by["126x22"].plan.last_rows, by["126x22"].plan.last_chunks) == (128, 84, 3)
    assert (by["502x11"].plan.rows, by["502x11"].plan.last_rows, by["502x11"].plan.last_chunks) == (192, 146, 5)


@pytest.mark.parametrize("row", BM.ROWS, ids=[r.name for r in BM.ROWS])
def test_rows_are_accepted_by_the_workspace_queries(row):
    lib = R.native.load()
    flags = (R.native.MODE_CORE if row.api == "render" else R.native.MODE_MVPS) | (R.native.FLAG_NO_ALBEDO if row.no_albedo else 0)
    for variant in (dict(), dict(deterministic=True)):
        d, n = _desc(row, **variant), C.c_int64(-1)
        assert lib.rnb_sample_workspace_bytes(C.byref(d), row.B, C.byref(n)) == 0 and n.value > 0, lib.rnb_last_error_string()
        n = C.c_int64(-1)
        assert lib.rnb_render_workspace_bytes(C.byref(d), row.B, row.S, flags, C.byref(n)) == 0 and n.value > 0, \
            lib.rnb_last_error_string()


# -------------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("row", BM.ROWS, ids=[r.name for r in BM.ROWS])
def test_restated_plan_is_the_librarys(row):
    got, want = library_plan(row), row.plan
    assert got["sdf_route"] == SDF_BF16
    assert got["color_route"] == (COLOR_BF16 if row.multires_view == 4 else COLOR_LAYERS)
    assert (got["njobs"], got["want"], got["rows"], got["splits"], got["total"]) == \
        (want.njobs, want.want, want.rows, want.splits, want.total)
    assert [tuple(j[2:5]) for j in got["jobs"]] == list(BM.JOBS[row.jobs_name])        # (K, lddw, npairs) in list order
    # the slabs of the deterministic variant lie one behind the other: [splits][256][lddw], then [splits][256]
    off = 0
    for j in got["jobs"]:
        assert j[8] == off
        off += want.splits * BM.N_ROWS * (j[3] + 1)
    assert off == want.total
    # the encoding columns of the albedo net's first layer are the one job without a bias and with a column offset
    assert [(j[6], j[7]) for j in got["jobs"]] == [(256, 0) if (j[0], j[2]) == (4, 64) else (0, 1) for j in got["jobs"]]


@pytest.mark.parametrize("row", BM.ROWS, ids=[r.name for r in BM.ROWS])
def test_the_flags_of_the_row_size_the_slabs_of_its_plan(row):
    """The deterministic variant adds ordered-reduction slabs to the render workspace (dw.hip dw_workspace_floats): those of the
    fp32 planner for the same descriptor (the dump tool's "slab_off" of a D line; its build answers 0 for the bf16 part) and
    the bf16 plan's total.  This ties the job count to the API flags of the row (FLAG_NO_ALBEDO: 8 jobs; `render`: 12),
    which a B line of the tool takes as a given."""
    lib = R.native.load()
    flags = (R.native.MODE_CORE if row.api == "render" else R.native.MODE_MVPS) | (R.native.FLAG_NO_ALBEDO if row.no_albedo else 0)
    size = {}
    for det in (False, True):
        n = C.c_int64(-1)
        assert lib.rnb_render_workspace_bytes(C.byref(_desc(row, deterministic=det)), row.B, row.S, flags, C.byref(n)) == 0
        size[det] = n.value
    d = _desc(row, deterministic=True)
    parts = "render(false,false)" if row.no_albedo else "render(true,false)"
    fp32 = json.loads(GEN.run(dump_tool(), [GEN.case_line(GEN._ints(d), int(d.variant), row.M, parts, 0)])[0])
    assert size[True] - size[False] == 4 * (fp32["slab_off"] + row.plan.total)
    assert size[True] - size[False] != 4 * (fp32["slab_off"] + BM.dw_plan(row.M, BM.JOBS["shipped" if row.jobs_name != "shipped" else "no_albedo"]).total)


def test_the_plan_moves_where_the_issue_says():
    """the restatement over a sweep of M, against the library's, for the three job lists (every 37th M up to 6000 and the
    neighbours of the first split-size change)"""
    ms = sorted(set(range(1, 6001, 37)) | {2751, 2752, 2753, 5504, 5505})
    lines, want = [], []
    for name, row in (("shipped", BM.BY_NAME["3x22"]), ("no_albedo", BM.BY_NAME["3x22_no_albedo"]), ("fp32_albedo", BM.BY_NAME["3x25_mv6"])):
        d = _desc(row)
        for m in ms:
            lines.append("B " + " ".join(str(x) for x in GEN._ints(d) + [int(d.variant), m, 0 if row.no_albedo else 1]))
            want.append(BM.dw_plan(m, BM.JOBS[name]))
    got = [json.loads(t) for t in GEN.run(dump_tool(), lines)]
    bad = [(w.M, w.njobs) for g, w in zip(got, want)
           if (g["njobs"], g["want"], g["rows"], g["splits"], g["total"]) != (w.njobs, w.want, w.rows, w.splits, w.total)]
    assert not bad, bad[:5]


# -------------------------------------------------------------------------------------------------------------- the tail
@functools.lru_cache(maxsize=None)
def sharp_params():
    import torch
    p = Golden("full_main_sharp").params()
    with torch.no_grad():
        p["dev.variance"].fill_(0.3)         # tests/bf16_emu_step.py model(sharpen=True)
    return p


@pytest.mark.parametrize("name", BM.TAIL_ROWS)
def test_the_last_k8_unit_holds_half_of_the_last_rays_weight(name):
    row = BM.BY_NAME[name]
    batch, z, pick = BM.tail_case(row, sharp_params())
    assert tuple(z.shape) == (row.B, row.S)
    share = BM.tail_share(row, sharp_params(), batch, z)
    print(f"BF16TAIL {name}: M = {row.M}, ray {pick} goes last, the last {row.tail} points hold {share:.3f} of its weights")
    assert share >= BM.TAIL_SHARE_MIN, f"{name}: the last K8 unit holds {share:.3f} of the last ray's weights"
