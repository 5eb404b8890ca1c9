"""The table of tests/point_matrix.py on the host (no GPU): the rows are the ones the table says, for each backward kind they
cover every class of weight-gradient job the one-workgroup kernel distinguishes, both sides of each forward-family boundary
appear, and the library's workspace query accepts every row for every flag set and variant tests/test_gpu_point_matrix.py uses.

The limit of this file: it needs nothing but the built library, and the split plan restated in tests/point_matrix.py
(dw_plan.h dw_staged_plan and dw_make_plan's room clamp) is no entry point of it.  What is pinned here is its slab room: the
plan's slab total in rnb_points_grad_workspace_bytes, as the difference between two rows of one padded size
(test_slab_room_matches_the_workspace_query).  The (job, split) layout itself meets the planner in
tests/test_dw_plan_host.py, which prints dw_make_plan's plan for the restated job shapes on the host (tools/dw_plan_dump.hip)
and compares it with plan_kind row by row; on the device it is met again through the route assertion of
tests/test_gpu_point_matrix.py (which kernel classes ran) and through the gradients those splits give."""
import ctypes as C

import pytest

import rnb_neus_fork_amd as R
from rnb_neus_fork_amd import runtime
from tests import point_matrix as PM
from tests import ray_matrix as RM


def _wide(plan):
    return [j for j in plan if j.width == 256]


def _narrow(plan):
    return [j for j in plan if j.width == 64]


def test_the_table_is_what_it_says():
    assert [r.M for r in PM.X3_ROWS] == [32, 64, 96, 128, 160, 1056, 2208, 2240, 3360, 8224]
    assert [r.M for r in PM.RAGGED_ROWS] == [33, 97, 127, 129, 2209, 8193, 32705]
    assert all(r.x3 and r.why for r in PM.X3_ROWS) and all(not r.x3 and r.why for r in PM.RAGGED_ROWS)
    assert set(PM.SHORT_ROWS) <= set(PM.BY_M) and {PM.BY_M[m].x3 for m in PM.SHORT_ROWS} == {True, False}
    assert PM.pad_rows(128) == 128 and PM.pad_rows(129) == 256 and PM.pad_rows(1) == 128
    # the job units of the default shape (dw_list): 7 wide jobs of 4 units and a narrow one of 2 with the normal, ...
    units = lambda jobs: sum(PM.job_units(n, w) for w, n in jobs)
    assert units(PM.KINDS["eikonal"].jobs) == 30 and units(PM.KINDS["feature"].jobs) == 17 and units(PM.KINDS["color"].jobs) == 5
    assert units(PM.KINDS["feature"].sized) == 32 and units(PM.KINDS["color"].sized) == 9
    assert all(len(k.jobs) <= PM.K_MAX_DW_JOBS for k in PM.KINDS.values())
    # what each row's `why` claims
    for kind in ("feature", "eikonal", "color"):
        for j in PM.plan(32, kind):
            assert (j.splits, j.last_rows) == (1, 32) and j.regimes == {"2"}
        for j in PM.plan(64, kind):
            assert (j.splits, j.last_rows) == (1, 64) and j.regimes == {"4"}
        for j in PM.plan(96, kind):
            assert (j.splits, j.rows, j.last_rows) == (2, 64, 32)
        for j in PM.plan(128, kind):
            assert (j.splits, j.rows, j.last_rows) == (2, 64, 64)
        for j in PM.plan(160, kind):
            assert (j.splits, j.rows, j.last_rows) == (3, 64, 32)
    eik = lambda m: {(j.splits, j.rows, j.last_rows) for j in _wide(PM.plan(m, "eikonal"))}
    assert eik(1056) == {(17, 64, 32)}
    assert eik(2208) == {(23, 96, 96)}
    assert eik(2240) == {(24, 96, 32)}
    assert eik(3360) == {(27, 128, 32)}
    assert eik(8224) == {(33, 256, 32)}
    clamped = [j for j in PM.plan(1056, "feature") if j.clamped]
    assert [(j.width, j.splits, j.rows, j.last_rows) for j in clamped] == [(256, 11, 96, 96)]
    assert {(j.width, j.splits, j.rows) for j in PM.plan(1056, "feature") if j.rows == 96} == {(256, 11, 96), (64, 11, 96)}
    assert [(j.splits, j.rows, j.last_rows) for j in PM.plan(8224, "color") if j.clamped] == [(65, 128, 32)]
    # the render steps: rays x S is the point count the test names
    sizes = [b * RM.BY_NAME[n].S for n, b, _ in PM.RENDER_STEPS]
    assert sizes == [726, 1056, 160] and not PM.runs_x3(726)


@pytest.mark.parametrize("kind", PM.KIND_NAMES)
def test_rows_cover_every_job_class(kind):
    """per backward kind: wide and narrow jobs; 2, 4, 6 and >= 8 chunks per split (on the wide body all four, on the narrow
    one at least the two short ones and the steady state); a full last split, a 32-row one behind full splits, one of an odd
    number of 32-row chunks; and the room clamp taken and not taken"""
    cov = PM.coverage(kind)
    for c in PM.WIDTH_CLASSES:
        assert cov.get(("width", c)), f"{kind}: no {c} job"
    for c in PM.REGIME_CLASSES:
        assert cov.get(("regime", c)), f"{kind}: no split of {c} chunks"
        assert cov.get(("wide regime", c)), f"{kind}: no wide job with a split of {c} chunks"
    for c in ("2", "4", ">=8"):
        assert cov.get(("narrow regime", c)), f"{kind}: no narrow job with a split of {c} chunks"
    for c in PM.LAST_CLASSES:
        assert cov.get(("last", c)), f"{kind}: no last split of class {c}"
    plans = [j for r in PM.X3_ROWS for j in PM.plan(r.M, kind)]
    # (the eikonal kind runs exactly the jobs its workspace was sized for: it never meets the clamp)
    assert any(j.clamped for j in plans) == (kind != "eikonal") and any(not j.clamped for j in plans)
    # a split is a whole number of 32-point chunks of at least 2 x 16 points, and the splits tile M exactly
    for r in PM.X3_ROWS:
        for j in PM.plan(r.M, kind):
            assert j.rows % PM.K_ST_CHUNK == 0 and j.last_rows % PM.K_ST_CHUNK == 0 and 0 < j.last_rows <= j.rows
            assert (j.splits - 1) * j.rows + j.last_rows == r.M
        assert sum(j.splits for j in PM.plan_kind(r.M, "eikonal")) <= 256, "one round of workgroups"


def test_forward_families():
    """both sides of each boundary of fused_forward's kernel families appear, each once with a ragged pad (M % 128 != 0)"""
    assert PM.forward_family(8192) == "32x8" and PM.forward_family(8193) == "32x4"
    assert PM.forward_family(32640) == "32x4" and PM.forward_family(32641) == "64x4"
    by_family = {}
    for r in PM.ROWS:
        by_family.setdefault(r.family, []).append(r.M)
    for below, above in PM.FAMILY_BOUNDARIES:
        for fam in (below, above):
            assert any(m % PM.K_ROW_PAD != 0 for m in by_family.get(fam, [])), f"no ragged row in family {fam}"
    assert PM.BY_M[8193].family == "32x4" and PM.BY_M[8193].Mp - 8193 == 127
    assert PM.BY_M[8224].family == "32x4" and 8224 - (PM.BY_M[8224].Mp - 128) == 32
    assert PM.BY_M[32705].family == "64x4" and 32705 % 64 == 1
    assert max(m for m in by_family["32x8"] if m % 128) == 3360


# ---------------------------------------------------------------------------------------------------------------------
# the workspace query
# ---------------------------------------------------------------------------------------------------------------------
def _nets():
    sdf = R.SDFNetwork(d_in=3, d_out=257, d_hidden=256, n_layers=8, skip_in=[4], multires=6)
    col = R.RenderingNetwork(d_feature=256, mode="no_view_dir", d_in=6, d_out=3, d_hidden=256, n_layers=2, multires_view=4)
    return sdf, col


def _desc(kind, **variant):
    """the descriptor the direct call of this kind builds (runtime._SDFPoints / _ColorPoints), with the variant bits"""
    sdf, col = _nets()
    d = runtime._color_desc(col, 256, 6) if kind == "color" else runtime.model_desc(sdf, None)
    d.variant = R.native.variant_bits(**variant)
    return d


def _flags(kind):
    return getattr(R.native, "POINTS_" + PM.KINDS[kind].flags)


def _grad_ws(d, n, flags):
    b = C.c_int64(-1)
    rc = R.native.load().rnb_points_grad_workspace_bytes(C.byref(d), n, flags, C.byref(b))
    assert rc == 0, R.native.load().rnb_last_error_string().decode()
    return b.value


VARIANTS = [dict(), dict(x2h=False), dict(deterministic=True)]


@pytest.mark.parametrize("variant", VARIANTS, ids=["default", "x2h=False", "deterministic"])
@pytest.mark.parametrize("kind", sorted(PM.KINDS))
def test_workspace_query_accepts_every_row(kind, variant):
    d = _desc(kind, **variant)
    rows = sorted(PM.ROWS, key=lambda r: (r.Mp, r.M))
    sizes = [_grad_ws(d, r.M, _flags(kind)) for r in rows]
    assert all(s > 0 for s in sizes)
    for (ra, a), (rb, b) in zip(zip(rows, sizes), zip(rows[1:], sizes[1:])):
        if rb.Mp > ra.Mp:
            assert b > a, f"{kind}: the workspace shrinks from M = {ra.M} (Mp {ra.Mp}) to M = {rb.M} (Mp {rb.Mp})"
    # non-decreasing in Mp over the whole table: the largest query of a padded size against the smallest of the next
    by_mp = {}
    for r, s in zip(rows, sizes):
        by_mp.setdefault(r.Mp, []).append(s)
    mps = sorted(by_mp)
    for a, b in zip(mps, mps[1:]):
        assert max(by_mp[a]) <= min(by_mp[b]), f"{kind}: workspace for Mp = {a} above that for Mp = {b}"


@pytest.mark.parametrize("kind", sorted(PM.KINDS))
def test_slab_room_matches_the_workspace_query(kind):
    """Two point counts of one padded size differ in the query by their weight-gradient slabs alone (every other buffer of
    carve_points is a function of Mp): the difference is 4 bytes x the difference of point_matrix.slab_room_floats, which
    pins the restated dw_staged_plan and the job lists dw_sizes sizes for, on the host."""
    d = _desc(kind)
    by_mp = {}
    for r in PM.ROWS:
        by_mp.setdefault(r.Mp, []).append(r.M)
    by_mp[PM.pad_rows(4096)] = [3999, 4000, 4064, 4096]     # (more splits than the small rows: rows per split vary here)
    checked = 0
    for mp, ms in by_mp.items():
        base = min(ms)
        for m in ms:
            want = 4 * (PM.slab_room_floats(m, PM.KINDS[kind]) - PM.slab_room_floats(base, PM.KINDS[kind]))
            got = _grad_ws(d, m, _flags(kind)) - _grad_ws(d, base, _flags(kind))
            assert got == want, f"{kind}: M = {m} against M = {base} (Mp {mp}): the query differs by {got} bytes, the table by {want}"
            checked += want != 0
    assert checked >= 3, "the rows of one padded size must differ in their slab room somewhere"
