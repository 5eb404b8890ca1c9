"""Workspace sizes of the bf16 route (RNB_VARIANT_BF16), no GPU: `rnb_render_workspace_bytes` against the sizes recorded
from the library of the commit before csrc/bf16.hip was split and the weight-gradient plan of its grouped launch
(bf16_dw.hip: jobs, splits, slab offsets, total) became one function — tests/golden/bf16_workspace_parent.json, written
by tools/gen_bf16_workspace_golden.py, which also holds the matrix.  The sizing of the deterministic variant's slabs
(`bf16_dw_floats`) and their carving in the launch now read the same plan; this test pins what that plan must total.

What a drift of the plan's total does to the byte count: every buffer of the workspace is carved in whole 256-byte units,
and the plan's total is a multiple of 256 floats (splits x 256 x (sum of row pitches + jobs)).  In every deterministic row
of the matrix the slab buffer ends on a 256-byte unit, so one float MORE moves the query by 256 bytes and the row fails
(tried once with `total + 1` compiled in: all 36 deterministic rows that carve the slabs failed).  One float LESS stays
inside the last unit and cannot be seen through the public query; a lost or mis-sized job is at least 256 floats."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_bf16_workspace_golden",
                                               os.path.join(ROOT, "tools", "gen_bf16_workspace_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "bf16_workspace_parent.json")))


def test_matrix_is_the_one_recorded():
    assert sorted(G.VARIANTS) == ["bf16", "bf16+deterministic"]
    assert sorted(G.SHAPES) == ["albedo3_mv4", "feature255", "shipped"]
    assert G.BS == (1, 37, 512) and G.SS == (128, 256)
    assert sorted(G.FLAGS) == ["mvps", "mvps|forward_only", "mvps|no_albedo"]
    assert len(G.cases()) == 2 * 3 * 3 * 2 * 3
    assert sorted(GOLDEN["bytes"]) == sorted(G.key(*c) for c in G.cases())
    assert GOLDEN["abi_version"] == G.N.ABI_VERSION == 5


@pytest.mark.parametrize("variant", list(G.VARIANTS))
@pytest.mark.parametrize("shape", list(G.SHAPES))
def test_workspace_bytes_equal_the_parents(variant, shape):
    d = G.desc(shape, variant)
    got = {G.key(variant, shape, B, S, f): G.workspace_bytes(d, B, S, G.FLAGS[f])
           for (v, sh, B, S, f) in G.cases() if (v, sh) == (variant, shape)}
    want = {k: GOLDEN["bytes"][k] for k in got}
    assert len(got) == 18
    assert got == want


def test_the_rows_differ_where_the_plan_does():
    """The recorded numbers are not one number: the deterministic variant adds slabs exactly where a backward runs, and the
    albedo route changes the job list."""
    b = GOLDEN["bytes"]
    for shape in G.SHAPES:
        for B in G.BS:
            for S in G.SS:
                k = lambda v, f: G.key(v, shape, B, S, f)
                assert b[k("bf16+deterministic", "mvps")] > b[k("bf16", "mvps")]
                assert b[k("bf16+deterministic", "mvps|no_albedo")] > b[k("bf16", "mvps|no_albedo")]
                assert b[k("bf16+deterministic", "mvps|forward_only")] == b[k("bf16", "mvps|forward_only")]
    k = lambda sh: G.key("bf16+deterministic", sh, 37, 256, "mvps")
    assert len({b[k(sh)] for sh in G.SHAPES}) == 3
