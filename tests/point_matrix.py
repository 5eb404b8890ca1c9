"""The point counts M of the point-tiled kernels of the shipped 256-wide route, with the code path each row exists for.

A plain module, like tests/ray_matrix.py: tests/test_point_matrix_host.py pins it on the host, tests/test_gpu_point_matrix.py
runs it on the device through the direct network calls (SDFNetwork / RenderingNetwork.set_autograd).  The kernels with edges
along M are the fused sweeps (fused.hip, fused_bwd.hip: 32- or 64-point tiles over Mp = pad_rows(M)), the two albedo sweeps
(color_h2.hip: 64-point tiles), and the weight gradients: gemm_dw_x3_kernel (dw.hip.h: one workgroup per (job, split), 16-point
chunks, "the raw rows run TWO chunks ahead in two register sets") with its split plan (dw.hip dw_staged_plan, held to the slab
room by dw_plan.h dw_make_plan) and dw_reduce_kernel, or, when M is no multiple of kStChunk = 32, the guarded split-K kernels.

This module restates in Python the three rules that decide a row's path; it needs no library:
  pad_rows            rnb_internal.h kRowPad
  forward_family      fused.hip fused_forward: "64-point tiles when that still gives every CU >= 2 workgroups, 32-point tiles
                      for small batches", 8 waves while there is "at most one workgroup per CU"
  staged_plan / plan  dw_plan.h dw_staged_plan and the one-workgroup loop of dw_make_plan over the jobs of dw_list, with the slab
                      room of its totals (DwPlan::slab_floats; tests/test_dw_plan_host.py holds both to the planner itself
                      through tools/dw_plan_dump.hip).  The job lists below are dw_list's for the descriptors the direct calls build
                      (runtime.py: model_desc(net, None) with a 32-wide placeholder albedo net, whose layers are no x3 jobs;
                      _color_desc(net, 256, 6) with a one-layer placeholder SDF net).

Backward kinds (KINDS): what one native backward runs.
  feature   rnb_sdf_backward, RNB_POINTS_FEATURE: the feature head and every hidden layer with ONE operand pair (zb_l / a_l-1);
            the workspace was sized for two pairs per hidden job, so layers 0 and 1 (the last the plan places) ask for more
            slabs than are left: `splits > room` in dw_make_plan, from M = 1056 on
  eikonal   rnb_sdf_backward, RNB_POINTS_NORMAL: every hidden layer with TWO pairs (gz_l / u_l and zb_l / in_l); the workspace
            is sized for exactly these jobs
  color     rnb_color_backward alone: three jobs (lin1; lin0 as a 256-column and a 64-column range) in a workspace sized
            for five; the two jobs it does not run leave room, and the clamp binds only for lin1 at M = 8224
  texture   Runner.validate_mesh_texture's chain: one backward of each kind above, in one autograd graph

Per job the kernel's software pipeline sees nchunks = rows / 16 of a split: the prologue loads chunks min(1, last) and
min(2, last), the loop body loads min(c + 3, last) and min(c + 4, last), and the bias column sum of the second register set is
guarded by `c + 2 < nchunks`: 2, 4, 6 and >= 8 chunks are different paths through those clamps, and the last split of a job
may be shorter than the others.
"""
from __future__ import annotations

from dataclasses import dataclass

K_ROW_PAD = 128        # rnb_internal.h kRowPad
K_ST_CHUNK = 32        # dw.hip.h kStChunk: a split is a whole number of these ("ranges are multiples of 32 points (host)")
K_X3_CHUNK = 16        # dw.hip.h kX3Chunk: the points of one pipeline stage of gemm_dw_x3_kernel
K_MAX_DW_JOBS = 12     # dw.hip.h kMaxDwJobs: one group of the one-workgroup kernel
N_ROWS = 256           # every x3 job has N = 256 rows (x3_job_shape)


def pad_rows(m: int) -> int:
    return (m + K_ROW_PAD - 1) // K_ROW_PAD * K_ROW_PAD


def runs_x3(m: int) -> bool:
    """dw_one_wg_runs on the default arithmetic: "only over whole 32-point chunks" """
    return m % K_ST_CHUNK == 0


def forward_family(m: int) -> str:
    """the kernel family of fused_forward for Mp = pad_rows(m): "32x8" (32-point tiles, 8 waves), "32x4", "64x4" """
    mp = pad_rows(m)
    small = mp // 64 < 512
    wide = mp // 32 <= 256
    return "64x4" if not small else ("32x8" if wide else "32x4")


FAMILY_BOUNDARIES = (("32x8", "32x4"), ("32x4", "64x4"))    # Mp <= 8192 | Mp < 32768 | above


def staged_plan(m: int, units: int, total_units: int):
    """dw_staged_plan: (splits, rows per split)"""
    splits = (256 * units) // total_units if total_units > 0 else 1
    splits = max(splits, 1)
    rows = (m + splits - 1) // splits
    rows = (rows + K_ST_CHUNK - 1) // K_ST_CHUNK * K_ST_CHUNK
    rows = max(rows, 2 * K_ST_CHUNK)
    return (m + rows - 1) // rows, rows


def job_units(npairs: int, width: int) -> int:
    """x3_job_units: "a 256-column pair costs about twice a narrow pair" """
    return npairs * (2 if width >= 256 else 1)


# (Y columns of the range, operand pairs) in dw_list's order; a K = 320 layer is x3_for_each_range's 256 + 64
_HIDDEN2 = [(256, 2)] * 7 + [(64, 2)]          # hidden layers 7 .. 1, then layer 0 (K = Ep = 64), with the normal
_HIDDEN1 = [(256, 1)] * 7 + [(64, 1)]          # ... without it
_FEAT = [(256, 1)]                             # the feature head
_ALBEDO = [(256, 1), (256, 1), (64, 1)]        # color.lin1; color.lin0 = 256 + 64 columns (Cinp = 320)


@dataclass(frozen=True)
class Kind:
    name: str
    flags: str          # the RNB_POINTS_* flag of the native call
    jobs: tuple         # the backward's x3 jobs (dw_list with its BwdParts)
    sized: tuple        # the jobs dw_workspace_floats sizes slabs for (BwdParts::render(with_color, false) on the call's descriptor)


KINDS = {
    # sized: the placeholder albedo net's layer (N = 32) is no x3 job; feature head + two pairs per hidden layer
    "feature": Kind("feature", "FEATURE", tuple(_FEAT + _HIDDEN1), tuple(_FEAT + _HIDDEN2)),
    "eikonal": Kind("eikonal", "NORMAL", tuple(_HIDDEN2), tuple(_HIDDEN2)),
    # sized: the albedo jobs, the feature head and the placeholder SDF net's one hidden layer (K = 64, two pairs)
    "color": Kind("color", "COLOR", tuple(_ALBEDO), tuple(_ALBEDO + _FEAT + [(64, 2)])),
}
TEXTURE_CHAIN = ("color", "eikonal", "feature")     # the order autograd runs the three backwards of the chain
KIND_NAMES = ("feature", "eikonal", "color", "texture")


@dataclass(frozen=True)
class JobPlan:
    kind: str
    width: int          # 256: wide; 64: narrow (dw_x3_chunk_narrow)
    npairs: int
    splits: int
    rows: int           # rows per split
    last_rows: int      # rows of the last split
    clamped: bool       # `splits > room` was taken

    @property
    def regimes(self) -> set:
        """the pipeline regimes the job's workgroups run: nchunks = 2, 4, 6 or >= 8 sixteen-point chunks, of the full splits
        and of the last one.  dw_staged_plan never plans a split below 64 rows ("if (rows < 2 * kStChunk)"), so the 2-chunk
        regime exists only as a 32-row LAST split (M = 32, or 32 rows behind full splits)"""
        name = lambda rows: {2: "2", 4: "4", 6: "6"}.get(rows // K_X3_CHUNK, ">=8")
        return ({name(self.rows)} if self.splits > 1 else set()) | {name(self.last_rows)}

    @property
    def last(self) -> set:
        """classes of the last split: "full"; "32behind": 32 rows behind at least one full split; "odd": an odd number of
        32-row chunks (an odd number of trips of the kernel's two-chunk loop)"""
        out = set()
        if self.last_rows == self.rows:
            out.add("full")
        if self.last_rows == K_ST_CHUNK and self.splits >= 2:
            out.add("32behind")
        if (self.last_rows // K_ST_CHUNK) % 2 == 1:
            out.add("odd")
        return out


def slab_room_floats(m: int, kind: Kind) -> int:
    """DwPlan::slab_floats of the sized jobs: the slab part of PointBufs::dw_part"""
    total = sum(job_units(n, w) for w, n in kind.sized)
    return sum(staged_plan(m, job_units(n, w), total)[0] * (N_ROWS * w + N_ROWS) for w, n in kind.sized)


def plan_kind(m: int, kind_name: str):
    """The (job, split) layout of one backward of `kind_name` over m points (a multiple of 32): the one-workgroup group of dw_make_plan."""
    assert runs_x3(m)
    kind = KINDS[kind_name]
    jobs = list(reversed(kind.jobs))          # "most recently produced operands first"
    assert len(jobs) <= K_MAX_DW_JOBS         # one group
    total = sum(job_units(n, w) for w, n in jobs)
    slab_left = slab_room_floats(m, kind)
    one_each = sum(N_ROWS * w + N_ROWS for w, _ in jobs)
    out = []
    for q, (w, n) in enumerate(jobs):
        splits, rows = staged_plan(m, job_units(n, w), total)
        per_split = N_ROWS * w + N_ROWS
        one_each -= per_split
        room = slab_left // per_split // (len(jobs) - q)
        if room < 1:
            room = (slab_left - one_each) // per_split
        assert room >= 1, "weight-gradient slab workspace exhausted"
        clamped = splits > room
        if clamped:
            splits = room
            rows = (m + splits - 1) // splits
            rows = (rows + K_ST_CHUNK - 1) // K_ST_CHUNK * K_ST_CHUNK
            splits = (m + rows - 1) // rows
        need = splits * per_split
        assert need <= slab_left, "weight-gradient slab workspace exhausted"
        slab_left -= need
        out.append(JobPlan(kind_name, w, n, splits, rows, m - (splits - 1) * rows, clamped))
    return out


def plan(m: int, kind_name: str):
    """every job of a backward kind over m points ("texture": the three backwards of the chain)"""
    if kind_name == "texture":
        return [j for k in TEXTURE_CHAIN for j in plan_kind(m, k)]
    return plan_kind(m, kind_name)


@dataclass(frozen=True)
class PointRow:
    M: int
    why: str

    @property
    def Mp(self) -> int:
        return pad_rows(self.M)

    @property
    def x3(self) -> bool:
        return runs_x3(self.M)

    @property
    def family(self) -> str:
        return forward_family(self.M)

    def __repr__(self):   # (pytest ids)
        return f"M{self.M}"


def _r(m, why):
    return PointRow(m, why)


X3_ROWS = [
    _r(32, "one split of 2 chunks in every job: last = 1, the prologue loads min(1, last) = 1 and min(2, last) = 1 (a re-read); "
           "`c + 2 < nchunks` is false on the only trip"),
    _r(64, "one split of 4 chunks: the loop's second trip loads min(c + 3, last) = min(c + 4, last) = 3"),
    _r(96, "two splits, 64 + 32 rows: a 2-chunk last split behind a full 4-chunk one"),
    _r(128, "Mp = M: no padded row anywhere; two full 64-row splits"),
    _r(160, "three splits, 64 + 64 + 32; the first row of the second 128-row pad"),
    _r(1056, "33 chunks of 32: 17 splits of 64 rows with a 32-row last split; the feature kind's layers 0 and 1, held to their "
             "slab room (`splits > room`), get 11 splits of exactly 96 rows (6 chunks)"),
    _r(2208, "eikonal wide jobs: 23 splits of exactly 96 rows (6 chunks, full last split)"),
    _r(2240, "eikonal wide jobs: 96-row splits with a 32-row last split"),
    _r(3360, "eikonal wide jobs: 128-row splits (8 chunks: the steady state of the two-ahead pipeline) with a 32-row last split"),
    _r(8224, "Mp = 8320: the first 128-row pad of the 4-wave forward family, 32 real rows in it; eikonal wide jobs: 33 splits of "
             "256 rows with a 32-row last split"),
]
RAGGED_ROWS = [
    _r(33, "one row past a chunk: the guarded split-K kernels; 31 dead rows in the fused sweeps' second 32-point tile"),
    _r(97, "one row past three chunks: the albedo sweeps' second 64-point tile holds 33 real rows"),
    _r(127, "one row short of the pad"),
    _r(129, "one real row in the second 128-row pad"),
    _r(2209, "one row past the 96-row-split row 2208"),
    _r(8193, "Mp = 8320: one real row beyond the 8-wave forward family"),
    _r(32705, "Mp = 32768: 64-point forward tiles, one real row in the last tile (32704 = 511 x 64)"),
]
ROWS = X3_ROWS + RAGGED_ROWS
BY_M = {r.M: r for r in ROWS}
assert len(BY_M) == len(ROWS), "point counts must be unique"

# the rows of the x2h=False and deterministic=True parametrizations, and of the render steps
SHORT_ROWS = [32, 96, 2240, 2209]
# (ray_matrix row, rays, batch step) of the render steps: M = rays x S
RENDER_STEPS = [("17+5/1", 33, 2), ("17+5/1", 48, 1), ("2+2/1", 40, 1)]

WIDTH_CLASSES = ("wide", "narrow")
REGIME_CLASSES = ("2", "4", "6", ">=8")
LAST_CLASSES = ("full", "32behind", "odd")


def coverage(kind_name: str):
    """{(class kind, class)} -> the point counts whose plan has a job of that class, over the x3 rows"""
    seen = {}
    for r in X3_ROWS:
        for j in plan(r.M, kind_name):
            wd = "wide" if j.width >= 256 else "narrow"
            keys = [("width", wd)] + [("regime", c) for c in j.regimes] + [(wd + " regime", c) for c in j.regimes]
            keys += [("last", c) for c in j.last]
            for k in keys:
                if r.M not in seen.setdefault(k, []):
                    seen[k].append(r.M)
    return seen
