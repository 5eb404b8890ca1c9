"""The point counts M = rays x samples of the bf16 route's backward (RNB_VARIANT_BF16, csrc/bf16_*.hip), with the code path
each row exists for.

A plain module, like tests/point_matrix.py (the fp32 route's table): tests/test_bf16_point_matrix_host.py pins it on the host,
tests/test_gpu_bf16_point_matrix.py runs it on the device.  The bf16 route keeps its per-point state in "K8" units (8
consecutive points of one column, 16 bytes), and every kernel with an edge along M works in these units or multiples of them:

  bf_dw_kernel        (bf16_dw.hip) one workgroup per (job, split).  Points >= M inside a unit are masked per bf16 pair
                      (bf_dw_mask_tail, X operand only); a step is 16 points (lane half h = 0 holds points 0..7, h = 1 points
                      8..15); K = 256 jobs walk 32-point chunks in a three-buffer LDS-DMA ring (chunks c + 1 and c + 2 in flight,
                      a chunk past the end is a re-fetch of the last), K = 64 jobs walk 16-point steps in a three-slot register ring
  bf_sdf_head_bwd_kernel, bf_color_out_bwd_kernel
                      guard `r + j < r1` inside a unit; bf_rows_per_slab rows per block (256 slabs, or ONE in the
                      deterministic variant)
  the sweeps          (bf16_sweeps.hip, bf16_color.hip) run over Mp = pad_rows(M) and read sbar / geb / fbar of the padded rows

This module restates the split plan of the grouped launch (bf16_dw_plan.h bf16_dw_shapes / bf16_dw_split; the host test
holds the restatement to the library's own plan through tools/dw_plan_dump.hip) and derives each row's classes from it.  It
needs no library.
"""
from __future__ import annotations

from dataclasses import dataclass, field

from oracle import rnb_oracle as O

K_ROW_PAD = 128          # rnb_internal.h kRowPad
K8 = 8                   # points of one K8 unit
K_STEP = 16              # points of one MFMA step of bf_dw_kernel
K_CHUNK = 32             # bf16_dw.hip kDwChunk: points of one LDS-ring chunk
K_SPLIT_ROWS = 64        # bf16_dw_plan.h kBfDwSplitRows
K_WANT = 512             # bf16_dw_plan.h kBfDwWant
N_ROWS = 256             # bf16_dw_plan.h kBfDwRows
K_SLABS = 256            # bf16_common.hip.h bf_rows_per_slab: row slabs of the head-backward kernels (1 when deterministic)


def _ceil(a: int, b: int) -> int:
    return (a + b - 1) // b


def pad_rows(m: int) -> int:
    return _ceil(m, K_ROW_PAD) * K_ROW_PAD


# (K, lddw, npairs) in bf16_dw_shapes' order, for the shipped SDF network (8 hidden layers, pe width 39 -> Ep = 64)
_HIDDEN = [(64, 64, 2)] + [(256, 256, 2)] * 7
_FEAT = [(256, 256, 1)]
_ALBEDO_BF16 = [(256, 256, 1), (256, 320, 1), (64, 320, 1)]      # color.lin1; color.lin0 as feature and encoding columns
JOBS = {
    "shipped": tuple(_HIDDEN + _FEAT + _ALBEDO_BF16),            # 12 jobs
    "no_albedo": tuple(_HIDDEN),                                 # 8: FLAG_NO_ALBEDO runs no colour backward
    "fp32_albedo": tuple(_HIDDEN + _FEAT),                       # 9: multires_view = 6, Cinp = 352 > 320: albedo dW in fp32
}


@dataclass(frozen=True)
class DwPlan:
    M: int
    njobs: int
    want: int
    rows: int            # points per split
    splits: int
    total: int           # floats of the deterministic variant's slabs

    @property
    def last_rows(self) -> int:
        return self.M - (self.splits - 1) * self.rows

    @property
    def full_chunks(self) -> int:
        """32-point chunks of a full split (0: there is none)"""
        return self.rows // K_CHUNK if self.splits > 1 else 0

    @property
    def last_chunks(self) -> int:
        return _ceil(self.last_rows, K_CHUNK)

    @property
    def last_steps(self) -> int:
        return _ceil(self.last_rows, K_STEP)


def dw_plan(m: int, jobs) -> DwPlan:
    """bf16_dw_split over the jobs of bf16_dw_shapes"""
    njobs = len(jobs)
    want = _ceil(K_WANT, njobs)
    rows = _ceil(_ceil(m, want), K_SPLIT_ROWS) * K_SPLIT_ROWS
    splits = _ceil(m, rows)
    total = sum(splits * N_ROWS * (lddw + 1) for _, lddw, _ in jobs)
    return DwPlan(m, njobs, want, rows, splits, total)


def tail_class(m: int) -> str:
    """M % 16: what bf_dw_mask_tail sees in the last step"""
    r = m % K_STEP
    return "0" if r == 0 else "1..7" if r < 8 else "8" if r == 8 else "9..15"


def rows_per_slab(m: int, deterministic: bool):
    """bf_rows_per_slab: (blocks, rows per block) of the two head-backward kernels"""
    slabs = 1 if deterministic else K_SLABS
    rows = _ceil(_ceil(m, slabs), K8) * K8
    return _ceil(m, rows), rows


def conf(n_samples, n_importance, steps):
    return O.RenderConf(n_samples=n_samples, n_importance=n_importance, up_sample_steps=steps)


@dataclass(frozen=True)
class Bf16Row:
    B: int
    render: O.RenderConf = field(compare=False)
    why: str = field(compare=False)
    api: str = "render_rnb"
    no_albedo: bool = False
    multires_view: int = 4          # 6: the fp32 albedo path behind the bf16 sweeps

    @property
    def S(self) -> int:
        return self.render.n_samples + self.render.n_importance

    @property
    def M(self) -> int:
        return self.B * self.S

    @property
    def Mp(self) -> int:
        return pad_rows(self.M)

    @property
    def jobs_name(self) -> str:
        if self.no_albedo:
            return "no_albedo"
        return "fp32_albedo" if self.multires_view != 4 else "shipped"

    @property
    def plan(self) -> DwPlan:
        return dw_plan(self.M, JOBS[self.jobs_name])

    @property
    def tail(self) -> int:
        """points of the last K8 unit"""
        return self.M % K8 or K8

    @property
    def model_conf(self) -> O.ModelConf:
        return O.ModelConf(color=O.ColorConf(multires_view=self.multires_view), render=self.render)

    @property
    def name(self) -> str:
        extra = ("_no_albedo" if self.no_albedo else "") + ("_render" if self.api == "render" else "") + \
            (f"_mv{self.multires_view}" if self.multires_view != 4 else "")
        return f"{self.B}x{self.S}{extra}"

    def __repr__(self):   # (pytest ids)
        return self.name


S22, S25, S16, S11 = conf(17, 5, 1), conf(20, 5, 1), conf(8, 8, 1), conf(8, 3, 1)

ROWS = [
    Bf16Row(1, S22, "M = 22: one split of one chunk: both ring prefetches are re-fetches of chunk 0.  M % 16 = 6: in the last "
                    "step the h = 0 half is partly masked, the h = 1 half wholly"),
    Bf16Row(3, S22, "M = 66: a full two-chunk split and a last split of 2 rows"),
    Bf16Row(3, S25, "M = 75: last split of 11 rows.  M % 16 = 11: the h = 1 half is partly masked, h = 0 not at all"),
    Bf16Row(172, S16, "M = 2752: 43 full splits of 64 rows: the largest grid of the shipped shape, the last M before a split "
                      "becomes 128 rows.  Mp - M = 64: half a pad of rows the sweeps run and no kernel may use"),
    Bf16Row(126, S22, "M = 2772: 128-row splits (4 chunks: the three-buffer ring wraps) and a last split of 84 rows = 3 "
                      "chunks, the last of them ragged"),
    Bf16Row(502, S11, "M = 5522: 192-row splits (6 chunks) and a last split of 146 rows = 5 chunks, the last ragged"),
    Bf16Row(3, S22, "M = 66 without the albedo net's backward: 8 jobs", no_albedo=True),
    Bf16Row(3, S22, "M = 66 through `render` (no lights, background colour)", api="render"),
    Bf16Row(3, S25, "M = 75 with multires_view = 6: 9 jobs; the albedo net runs in fp32 behind the bf16 sweeps, so FB reads "
                    "the fp32 fbar of the padded rows", multires_view=6),
]
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS), "row names must be unique"

DETERMINISTIC_ROWS = ["1x22", "3x25", "126x22", "502x11"]       # one block per head-backward kernel, ordered slabs
TAIL_ROWS = ["3x22", "3x25", "126x22", "502x11"]                # the last K8 unit made to carry half a gradient
POISON_ROWS = ["3x25", "126x22"]                                # padded rows never reach a result

TAIL_SHARE_MIN = 0.5     # of the last ray's `weights` sum, on the last K8 unit's points (fp64 oracle)
TAIL_KEY = "sdf.lin1.weight_v"


# ---------------------------------------------------------------------------------------------------------------------
# the tail made to matter: a ray that hits the surface goes last, its last depths straddle the hit
# ---------------------------------------------------------------------------------------------------------------------
def row_batch(row: Bf16Row):
    """the rays of tests/bf16_emu_step.step for this row"""
    return O.synthetic_batch(row.B, seed=40 + row.B, step=1, warmup=False)


def hit_depths(p, mc, batch, n_probe=129):
    """per ray: the depth of the first outside -> inside crossing of the fp64 oracle's SDF on n_probe uniform depths (linear
    interpolation), NaN where the ray starts inside or never crosses"""
    import torch
    q = {k: v.detach().double() for k, v in p.items()}
    o, d = batch["rays_o"].double(), batch["rays_d"].double()
    near, far = batch["near"].double(), batch["far"].double()
    t = near + (far - near) * torch.linspace(0.0, 1.0, n_probe, dtype=torch.float64)[None, :]
    pts = o[:, None, :] + d[:, None, :] * t[..., None]
    with torch.no_grad():
        sdf = O.sdf_only(q, mc.sdf, pts.reshape(-1, 3)).reshape(t.shape)
    cross = (sdf[:, :-1] > 0) & (sdf[:, 1:] <= 0)
    first = torch.argmax(cross.to(torch.int32), dim=1)
    ok = cross.any(dim=1) & (sdf[:, 0] > 0)      # (from a positive start the first crossing is the first non-positive probe)
    i = first[:, None]
    s0, s1, t0, t1 = sdf.gather(1, i), sdf.gather(1, i + 1), t.gather(1, i), t.gather(1, i + 1)
    hit = (t0 + (t1 - t0) * s0 / (s0 - s1))[:, 0]
    return torch.where(ok, hit, torch.full_like(hit, float("nan")))


def tail_case(row: Bf16Row, p):
    """(batch with the chosen ray last, z_vals [B, S] fp32, index the ray had): the first ray of row_batch that is inside
    the mask (its colour term is live), starts outside the surface and hits it in the middle half of (near, far).  Its first
    S - tail depths are squeezed into [near, near + 0.05 (t* - near)], its last `tail` depths straddle t* by +- 0.1 (far - near);
    every other ray takes uniform depths."""
    import torch
    mc, B, S, tail = row.model_conf, row.B, row.S, row.tail
    batch = row_batch(row)
    near, far = batch["near"].double()[:, 0], batch["far"].double()[:, 0]
    hit = hit_depths(p, mc, batch)
    span = far - near
    good = torch.isfinite(hit) & (hit > near + 0.25 * span) & (hit < far - 0.25 * span) & (batch["mask"][:, 0] > 0.5)
    assert bool(good.any()), f"{row.name}: no ray of the batch hits the surface in the middle half of its depth range"
    pick = int(torch.nonzero(good)[0])
    order = [i for i in range(B) if i != pick] + [pick]
    per_ray = {"rays_o": 0, "rays_d": 0, "near": 0, "far": 0, "t_rand": 0, "mask": 0, "true_rgb": 1, "lights_dir": 1}
    out = {k: v.index_select(per_ray[k], torch.tensor(order)).contiguous() for k, v in batch.items()}
    u = torch.linspace(0.0, 1.0, S, dtype=torch.float64)
    z = out["near"].double() + (out["far"].double() - out["near"].double()) * u[None, :]
    n0, f0, t0 = float(near[pick]), float(far[pick]), float(hit[pick])
    head = n0 + 0.05 * (t0 - n0) * torch.linspace(0.0, 1.0, S - tail, dtype=torch.float64)
    last = t0 + 0.1 * (f0 - n0) * (torch.linspace(-1.0, 1.0, tail, dtype=torch.float64) if tail > 1 else torch.zeros(1, dtype=torch.float64))
    z[B - 1] = torch.cat([head, last])
    assert bool((z[:, 1:] > z[:, :-1]).all())
    return out, z.float().contiguous(), pick


def tail_share(row: Bf16Row, p, batch, z):
    """the share of the last ray's `weights` that the points of the last K8 unit hold, in the fp64 oracle"""
    import torch
    q = {k: v.detach().double() for k, v in p.items()}
    b = {k: v.double() for k, v in batch.items()}
    with torch.enable_grad():
        out = O.render_rnb(q, row.model_conf, b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"],
                           cos_anneal_ratio=1.0, z_vals=z.double())
    w = out["weights"].detach()[-1]
    return float(w[row.S - row.tail:].sum() / w.sum())


def weighted_rnb_loss(out, true_rgb, mask, rw, igr_weight=0.1, mask_weight=0.1):
    """O.rnb_loss with ray b's colour and mask terms times rw[b]; rw = 1 is O.rnb_loss.  (The eikonal term is one mean over
    all points: it keeps its weight.)"""
    import torch
    dt = out["weight_sum"].dtype
    rw = rw.to(dtype=dt, device=out["weight_sum"].device).reshape(-1)
    m = (mask > 0.5).to(dt)
    n_lights = true_rgb.shape[0]
    col = ((out["color_fine"] - true_rgb).abs() * m[None, :, :]).sum(dim=(0, 2)) / ((m.sum() + 1e-5) * n_lights)
    ws = out["weight_sum"].clip(1e-3, 1.0 - 1e-3)
    bce = -(m * torch.log(ws) + (1.0 - m) * torch.log(1.0 - ws))[:, 0] / m.shape[0]
    return (rw * (col + mask_weight * bce)).sum() + igr_weight * out["gradient_error"]
