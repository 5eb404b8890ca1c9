"""The sample and light counts of the per-ray kernels ("one wave64 per ray": sampling.hip, composite.hip, train.hip), with
the code path each row exists for.

A plain module, like tests/shape_matrix.py: tests/test_ray_matrix_host.py pins it on the host (every accepted row is
accepted by the workspace queries and resolved by the oracle, every refused row the queries can see is refused by them),
tests/test_gpu_ray_matrix.py runs it on the device.  These kernels read their sizes at run time and walk a ray in 64-lane
pieces with a carry between pieces, so the rows sit where such a kernel goes wrong without a 64-aligned case noticing:
odd `n` (linspace_at's second half), n_new = 1 and n_new = kMaxNew = 64, `per = ceil((n - 1) / 64)` just above and below a
multiple of 64, n + n_new = kMaxZ = 512, S = kMaxS = 512, and S with a carry followed by a ragged chunk.

Per row:
  n_samples + n_importance / up_sample_steps   the RenderConf
  n_lights    lights of the render_rnb step (the library holds them in registers: kMaxRenderLights = 8)
  z_vals_S    > 0: the row is a render at S explicit depths (no sampling); its S is this, not n_samples + n_importance
  accepted    False: the library must refuse the row; `refused_by` says where ("sample_query": rnb_sample_workspace_bytes,
              "render_query": rnb_render_workspace_bytes, "call": only the render call sees it) and `limit` is a word the
              error message must contain
  why         the code path, in the words of the kernel source
"""
from __future__ import annotations

from dataclasses import dataclass

from oracle import rnb_oracle as O

K_MAX_NEW, K_MAX_Z, K_MAX_S, K_MAX_LIGHTS = 64, 512, 512, 8    # sampling.hip / composite.hip (rnb_internal.h)


@dataclass(frozen=True)
class RayRow:
    n_samples: int
    n_importance: int
    up_sample_steps: int
    n_lights: int
    why: str
    accepted: bool = True
    refused_by: str = ""
    limit: str = ""
    z_vals_S: int = 0

    @property
    def n_new(self) -> int:
        """new depths per up-sampling step (0: no importance sampling)"""
        return self.n_importance // self.up_sample_steps if self.n_importance > 0 else 0

    @property
    def S(self) -> int:
        return self.z_vals_S if self.z_vals_S > 0 else self.n_samples + self.n_importance

    @property
    def step_n(self):
        """`n` (depths on the ray) entering every up-sampling step"""
        if self.n_importance <= 0:
            return []
        return [self.n_samples + i * self.n_new for i in range(self.up_sample_steps)]

    @property
    def name(self) -> str:
        base = f"{self.n_samples}+{self.n_importance}"
        if self.n_importance > 0:
            base += f"/{self.up_sample_steps}"
        if self.z_vals_S:
            base = f"z{self.z_vals_S}"
        return base + (f"_L{self.n_lights}" if self.n_lights != 3 else "")

    @property
    def render_conf(self) -> O.RenderConf:
        return O.RenderConf(n_samples=self.n_samples, n_importance=self.n_importance, up_sample_steps=self.up_sample_steps)

    def __repr__(self):   # (pytest ids)
        return self.name


def _r(ns, ni, steps, why, L=3, **kw):
    return RayRow(ns, ni, steps, L, why, **kw)


BASE_ROWS = [
    _r(2, 0, 1, "S = 2: z_init_kernel's linspace_at with steps = 2 (one element per half); composite: two live lanes, "
                "sample S-1 re-read on 62 idle lanes; the z_bar stencil with no interior sample"),
    _r(2, 2, 1, "n = 2: m = n - 1 = 1 section, per = 1, j0 = j1 on 63 lanes; n_new = 2"),
    _r(3, 3, 3, "n_new = 1 on every step: linspace_at's `steps == 1` case gives u = 0.5; odd n = 3 (steps / 2 = 1)"),
    _r(5, 40, 8, "eight steps with n_new = n_samples = 5 (the largest the reference's ratio allows); odd n on every other step"),
    _r(17, 5, 1, "odd n = 17, odd n_new = 5: both linspace_at calls take `i < steps / 2` on fewer than half the elements"),
    _r(63, 63, 1, "n = 63: m = 62 < 64, per = 1 with two empty lanes; n_new = 63 = one idle lane in `lane < n_new`"),
    _r(64, 0, 1, "S = 64: exactly one full chunk, no carry, no idle lane"),
    _r(65, 0, 1, "S = 65: the smallest carry followed by a ragged chunk (one live lane, 63 re-reading sample S-1)"),
    _r(65, 64, 1, "n = 65: m = 64, per = 1 with every lane loaded; n_new = kMaxNew = 64; S = 129 = two chunks + one lane"),
    _r(66, 21, 3, "n = 66: m = 65, per = 2, lanes 33..63 empty (j0 = j1 = m); n_new = 7 odd; S = 87"),
    _r(100, 90, 2, "n_new = 45; n = 100, 145: per = 2 and 3 with a part-filled last segment; S = 190 = two chunks + 62 lanes"),
    _r(127, 64, 1, "n = 127: m = 126, per = 2, 63 full lanes; n_new = 64; S = 191"),
    _r(129, 39, 3, "n = 129, 142, 155 (per = 2, 3, 3), n_new = 13; S = 168; two of the three steps merge an odd n"),
    _r(191, 192, 3, "n_new = 64 three times (n = 191, 255, 319: per = 3, 4, 5); S = 383 = five chunks + 63 lanes"),
    _r(448, 64, 1, "n + n_new = kMaxZ = 512 in one step: n = 448, per = 7; the rank-count merge over 512 slots"),
    _r(64, 448, 7, "seven steps at n_new = 64 from n = 64 to n + n_new = 512: every LDS row of up_sample_kernel filled once"),
    _r(256, 256, 4, "every step at n_new = 64, last step n + n_new = 512; S = kMaxS = 512: eight full chunks of the composite"),
]

# light counts 1, 2, 5 and the limit 8 (Lv[kMaxL][3] / col[kMaxL][4] in registers) on a row with S < 64 and on one with a
# carry and a ragged chunk
_LIGHT_BASE = {"2+0": "S = 2 < 64", "65+64/1": "S = 129: a carry and a ragged chunk"}
LIGHT_ROWS = [
    _r(b.n_samples, b.n_importance, b.up_sample_steps,
       f"{L} light{'s' if L > 1 else ''}{' = kMaxRenderLights' if L == 8 else ''} at {_LIGHT_BASE[b.name]}", L=L)
    for b in BASE_ROWS if b.name in _LIGHT_BASE for L in (1, 2, 5, 8)
]

REFUSED_ROWS = [
    _r(4, 16, 2, "n_new = 8 > n_samples = 4: check_sampling_desc (the reference's ratio)", accepted=False,
       refused_by="sample_query", limit="n_samples"),
    _r(16, 10, 4, "n_importance % up_sample_steps != 0", accepted=False, refused_by="sample_query", limit="multiple"),
    _r(1, 0, 1, "n_samples = 1: linspace over one depth has no step", accepted=False, refused_by="sample_query", limit=">= 2"),
    _r(128, 65, 1, "n_new = 65 > kMaxNew: more new depths than lanes", accepted=False, refused_by="sample_query", limit="kMaxNew"),
    _r(449, 64, 1, "n + n_new = 513 > kMaxZ: past the LDS rows of up_sample_kernel", accepted=False, refused_by="sample_query",
       limit="kMaxZ"),
    _r(16, 16, 4, "S = 513 > kMaxS by explicit z_vals: past the LDS rows of composite_bwd_body", accepted=False,
       refused_by="render_query", limit="kMaxS", z_vals_S=513),
    _r(16, 16, 4, "9 lights > kMaxRenderLights: a property of the call, not of the descriptor", L=9, accepted=False,
       refused_by="call", limit="kMaxRenderLights"),
]

ROWS = BASE_ROWS + LIGHT_ROWS + REFUSED_ROWS
ACCEPTED = [r for r in ROWS if r.accepted]
REFUSED = [r for r in ROWS if not r.accepted]
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS), "row names must be unique"

# the rows that also run on the fused sweeps (default_64x64, 64 rays: B * S is not a multiple of 64 in most of them)
FUSED_ROW_NAMES = ["2+0", "17+5/1", "65+64/1", "129+39/3", "64+448/7", "256+256/4"]
BF16_ROW_NAMES = ["65+64/1", "129+39/3", "64+448/7"]
# explicit depths: S of the forward-only renders, and of the z_vals.grad cases
Z_VALS_S = [1, 2, 63, 65, 100, 129, 190, 511, 512]
Z_GRAD_S = [2, 63, 65, 129, 190]
# every float output of a render (the explicit-depth forwards check each; the input-gradient cases weight each in their loss)
FLOAT_OUTS = ("color_fine", "s_val", "cdf_fine", "weight_sum", "weight_max", "gradients", "weights", "gradient_error")


def up_sample_pairs():
    """every distinct (n, n_new) an accepted row sends to up_sample_kernel, sorted"""
    return sorted({(n, r.n_new) for r in ACCEPTED for n in r.step_n})


# ---------------------------------------------------------------------------------------------------------------------
# inputs and the reference of the up_sample_kernel tests (shared by the host and the device test)
# ---------------------------------------------------------------------------------------------------------------------
UP_RAYS = 48
UP_INV_S = (64.0, 512.0)


def up_sample_inputs(n, rays=UP_RAYS, seed=0):
    """rays_o, rays_d, sorted non-uniform depths [rays, n] between near and far of O.synthetic_batch, and the SDF row
    |p| - 0.5 + 0.02 sum sin(7 p) at them"""
    import torch
    b = O.synthetic_batch(rays, seed=5, step=2, warmup=False)
    gen = torch.Generator().manual_seed(100003 * n + seed)
    u = torch.rand(rays, n, generator=gen)
    z = torch.sort(b["near"] + (b["far"] - b["near"]) * u, dim=-1).values.contiguous()
    return b["rays_o"].contiguous(), b["rays_d"].contiguous(), z, analytic_sdf(b["rays_o"], b["rays_d"], z)


def analytic_sdf(rays_o, rays_d, z):
    import torch
    p = rays_o[:, None, :] + rays_d[:, None, :] * z[..., None]
    return (torch.linalg.norm(p, dim=-1) - 0.5 + 0.02 * torch.sin(7.0 * p).sum(-1)).contiguous()


def up_sample_cdf_reexpressed(rays_o, rays_d, z, sdf, inv_s):
    """The CDF of O.up_sample / O.sample_pdf_det in fp32 with the two things the kernel does differently: the sigmoid written
    1 / (1 + exp(-x)) (expf against torch.sigmoid) and the normaliser summed sequentially in double (torch.sum's order).
    Everything else rounds where the oracle rounds."""
    import torch
    B, n = z.shape
    pts = rays_o[:, None, :] + rays_d[:, None, :] * z[..., :, None]
    radius = torch.linalg.norm(pts, ord=2, dim=-1)
    inside = (radius[:, :-1] < 1.0) | (radius[:, 1:] < 1.0)
    prev_sdf, next_sdf = sdf[:, :-1], sdf[:, 1:]
    prev_z, next_z = z[:, :-1], z[:, 1:]
    mid_sdf = (prev_sdf + next_sdf) * 0.5
    cos_val = (next_sdf - prev_sdf) / (next_z - prev_z + 1e-5)
    prev_cos = torch.cat([torch.zeros([B, 1]), cos_val[:, :-1]], dim=-1)
    cos_val = torch.minimum(prev_cos, cos_val).clip(-1e3, 0.0) * inside
    dist = next_z - prev_z

    def sig(x):
        return 1.0 / (1.0 + torch.exp(-x))

    prev_cdf = sig((mid_sdf - cos_val * dist * 0.5) * inv_s)
    next_cdf = sig((mid_sdf + cos_val * dist * 0.5) * inv_s)
    alpha = (prev_cdf - next_cdf + 1e-5) / (prev_cdf + 1e-5)
    trans = torch.cumprod(torch.cat([torch.ones([B, 1]), 1.0 - alpha + 1e-7], -1), -1)[:, :-1]
    w = alpha * trans + 1e-5
    tot = torch.zeros(B, dtype=torch.float64)
    for j in range(w.shape[1]):          # sequential, in double
        tot = tot + w[:, j].double()
    pdf = w / tot.float()[:, None]
    cdf = torch.cumsum(pdf, -1)
    return torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)


def near_tie_exempt(cdf, cdf2, n_new):
    """(exempt mask [B, n_new], margin): a sample is exempt from the exact-index check when some cdf[k] lies within
    margin = 2 max|cdf - cdf'| of its u (2 x: both neighbours of u move)"""
    import torch
    margin = 2.0 * float((cdf.double() - cdf2.double()).abs().max())
    u = torch.linspace(0.5 / n_new, 1.0 - 0.5 / n_new, steps=n_new).double()
    d = (cdf.double()[:, :, None] - u[None, None, :]).abs().amin(dim=1)
    return d <= margin, margin


def up_sample_reference(n, n_new, inv_s, dtype=None, rays=UP_RAYS):
    """O.up_sample with a trace on up_sample_inputs(n): dict(new_z, inds, cdf, z, sdf, rays_o, rays_d) in `dtype` (fp32)."""
    import torch
    ro, rd, z, sdf = up_sample_inputs(n, rays)
    dt = dtype or torch.float32
    tr = {}
    new_z = O.up_sample(ro.to(dt), rd.to(dt), z.to(dt), sdf.to(dt), n_new, inv_s, tr)
    return dict(new_z=new_z, inds=tr["inds"], cdf=tr["cdf"], z=z, sdf=sdf, rays_o=ro, rays_d=rd)
