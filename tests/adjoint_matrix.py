"""The cotangents of a render (`rnb_render_grads`: color_fine, weights, cdf_fine, gradients, weight_sum, weight_max, s_val,
gradient_error), one at a time, with everything a parameter-gradient comparison against fp64 needs fixed BEFORE any device
code runs.

A plain module, like tests/ray_matrix.py: tests/test_adjoint_matrix_host.py pins it on the CPU oracle (the declared zero
leaves are the oracle's zero leaves, every other leaf is a parity target, the weight_max selection keeps enough rays and
the fp32 oracle agrees with fp64 on their arg-max), tests/test_gpu_adjoint_matrix.py runs it on the device.

Rows are (shape, api, adjoint).  `adjoint` is one output name, or "all" for the eight together.  `api`:
  render                 background_rgb = [0.2, 0.5, 0.8]
  render_rnb             per-ray lights [L, B, 1, 3]
  render_rnb_warmup      shared lights [L, 1, 1, 3], ReLU on the shading
  render_rnb_no_albedo   render_rnb(no_albedo=True): the albedo network is not a leaf of the call (color_fine only)
Every render runs at cos_anneal_ratio = 0.5 (both terms of the composite's tcbar live) and at explicit depths: `depths()`
is O.sample_rays in fp32 on the CPU at 64 + 16 samples in one up-sampling step, S = 80 = one carry and a ragged 16-lane
chunk of the per-ray kernels, handed as z_vals= to the device and to both oracles.

Shapes:
  w32             the per-layer path, 16 rays of O.synthetic_batch(16, seed=11, step=1)
  default_64x64   the fused sweeps and the h2 albedo kernels, 64 rays of step 2 (weight_sum mean 0.55; with 16 rays this
                  state falls under gpu_support.assert_has_surface, see tests/test_gpu_ray_matrix.py)

Cotangents: for every output a fixed-seed randn / sqrt(numel), drawn for all eight in the order of ray_matrix.FLOAT_OUTS
whatever the row's adjoint is, so "all" is the sum of the single rows.

The weight_max cotangent.  max over a ray's weights is not differentiable where the top two weights tie, and a ray that
misses the surface has every weight ~1e-5: its arg-max is arbitrary.  The cotangent is therefore non-zero only on the rays
whose fp64 top-two gap exceeds  2 x parity.value_bound(w64, max|w32 - w64|)  — the project's output rule: two samples that
each move by at most the device's allowed error cannot swap.  Measured on the CPU oracle (pinned by the host test to stay
at or above half of the rays; the margin moves with the host's fp32 arithmetic, the counts were the same on two hosts):
  w32             15 of 16 rays kept (max|w32 - w64| 5.9e-07 .. 6.9e-07, margin 7.5e-06 .. 8.1e-06)
  default_64x64   53 of 64 rays kept (max|w32 - w64| 6.7e-07 .. 1.1e-06, margin 8.0e-06 .. 1.05e-05)

Structural zeros.  A rel-L2 rule divides by zero on a leaf the adjoint cannot reach; those leaves are written out by name
below (ZERO_LEAVES) and held to exactly 0.0 on the device:
  the albedo network under every adjoint except color_fine (no colour, no albedo), and under color_fine with no_albedo;
  every leaf except dev.variance under s_val (s_val = 1 / inv_s);
  dev.variance, the albedo network and the last SDF layer's bias under gradients and gradient_error (the normal is a
  derivative of the SDF with respect to the point: a constant offset of the output drops out, inv_s never enters).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, replace

import torch

from oracle import rnb_oracle as O
from tests import parity as P
from tests.ray_matrix import FLOAT_OUTS
from tests.shape_matrix import BY_NAME as SHAPE_BY_NAME, live_params

RENDER = O.RenderConf(n_samples=64, n_importance=16, up_sample_steps=1)
S = RENDER.n_samples + RENDER.n_importance
COS_ANNEAL = 0.5
BACKGROUND = (0.2, 0.5, 0.8)
COT_SEED = 5
# shape -> (rays, step of O.synthetic_batch(seed=11))
RAYS = {"w32": (16, 1), "default_64x64": (64, 2)}
APIS = ("render", "render_rnb", "render_rnb_warmup", "render_rnb_no_albedo")
ADJOINTS = ("color_fine", "weights", "cdf_fine", "gradients", "weight_sum", "weight_max", "s_val", "gradient_error")
assert set(ADJOINTS) == set(FLOAT_OUTS)


@dataclass(frozen=True)
class AdjRow:
    shape: str
    api: str
    adjoint: str

    @property
    def name(self) -> str:
        return f"{self.shape}-{self.api}-{self.adjoint}"

    @property
    def outputs(self):
        """the outputs that carry a cotangent"""
        return ADJOINTS if self.adjoint == "all" else (self.adjoint,)

    def __repr__(self):   # (pytest ids)
        return self.name


ROWS = (
    [AdjRow("w32", api, adj) for api in APIS[:3] for adj in ADJOINTS]
    + [AdjRow("w32", "render_rnb_no_albedo", "color_fine")]
    + [AdjRow("default_64x64", "render_rnb", adj) for adj in ADJOINTS + ("all",)]
    + [AdjRow("default_64x64", "render", adj) for adj in ("color_fine", "s_val", "weight_max")]
)
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS), "row names must be unique"

# ---------------------------------------------------------------------------------------------------------------------
# the leaves no cotangent of the row reaches, by name (both shapes: eight hidden SDF layers, two hidden albedo layers)
# ---------------------------------------------------------------------------------------------------------------------
ALBEDO_LEAVES = frozenset((
    "color.lin0.bias", "color.lin0.weight_g", "color.lin0.weight_v",
    "color.lin1.bias", "color.lin1.weight_g", "color.lin1.weight_v",
    "color.lin2.bias", "color.lin2.weight_g", "color.lin2.weight_v",
))
SDF_LEAVES = frozenset((
    "sdf.lin0.bias", "sdf.lin0.weight_g", "sdf.lin0.weight_v",
    "sdf.lin1.bias", "sdf.lin1.weight_g", "sdf.lin1.weight_v",
    "sdf.lin2.bias", "sdf.lin2.weight_g", "sdf.lin2.weight_v",
    "sdf.lin3.bias", "sdf.lin3.weight_g", "sdf.lin3.weight_v",
    "sdf.lin4.bias", "sdf.lin4.weight_g", "sdf.lin4.weight_v",
    "sdf.lin5.bias", "sdf.lin5.weight_g", "sdf.lin5.weight_v",
    "sdf.lin6.bias", "sdf.lin6.weight_g", "sdf.lin6.weight_v",
    "sdf.lin7.bias", "sdf.lin7.weight_g", "sdf.lin7.weight_v",
    "sdf.lin8.bias", "sdf.lin8.weight_g", "sdf.lin8.weight_v",
))
VARIANCE = "dev.variance"
_NORMAL_ONLY = ALBEDO_LEAVES | {VARIANCE, "sdf.lin8.bias"}
_BY_ADJOINT = {
    "color_fine": frozenset(),
    "weights": ALBEDO_LEAVES,
    "cdf_fine": ALBEDO_LEAVES,
    "weight_sum": ALBEDO_LEAVES,
    "weight_max": ALBEDO_LEAVES,
    "gradients": _NORMAL_ONLY,
    "gradient_error": _NORMAL_ONLY,
    "s_val": ALBEDO_LEAVES | SDF_LEAVES,
    "all": frozenset(),
}
ZERO_LEAVES = {(api, adj): z for api in APIS[:3] for adj, z in _BY_ADJOINT.items()}
ZERO_LEAVES[("render_rnb_no_albedo", "color_fine")] = ALBEDO_LEAVES


def zero_leaves(row: AdjRow):
    return ZERO_LEAVES[(row.api, row.adjoint)]


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model(shape: str):
    """(ModelConf at the matrix's RenderConf, named parameters on the CPU) of a shape of tests/shape_matrix.py"""
    sh = SHAPE_BY_NAME[shape]
    mc = replace(sh.mc, render=RENDER)
    return mc, live_params(mc, sh.seed)


def batch(shape: str, api: str):
    B, step = RAYS[shape]
    return O.synthetic_batch(B, seed=11, step=step, warmup=api == "render_rnb_warmup")


@functools.lru_cache(maxsize=None)
def depths(shape: str):
    """the explicit depths [B, S] of every row of the shape: the fp32 oracle's own sampling (no device code)"""
    mc, p = model(shape)
    b = batch(shape, "render_rnb")
    with torch.no_grad():
        z = O.sample_rays(p, mc, b["rays_o"], b["rays_d"], b["near"], b["far"], b["t_rand"], 1.0)
    assert tuple(z.shape) == (RAYS[shape][0], S)
    return z.contiguous()


def oracle_render(shape: str, api: str, q, dt):
    """the oracle's render of `api` with the parameters q (already of dtype dt) at depths(shape)"""
    b = {k: v.to(dt) for k, v in batch(shape, api).items()}
    mc, _ = model(shape)
    z = depths(shape).to(dt)
    if api == "render":
        return O.render(q, mc, b["rays_o"], b["rays_d"], b["near"], b["far"], background_rgb=torch.tensor(BACKGROUND, dtype=dt),
                        cos_anneal_ratio=COS_ANNEAL, z_vals=z)
    return O.render_rnb(q, mc, b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=COS_ANNEAL,
                        warmup=api == "render_rnb_warmup", no_albedo=api == "render_rnb_no_albedo", z_vals=z)


@functools.lru_cache(maxsize=None)
def _oracle_forward(shape: str, api: str, dt):
    """(leaves, outputs with their graph): one forward per (shape, api, dtype), shared by every adjoint of it"""
    _, p = model(shape)
    q = {k: v.detach().to(dt).requires_grad_(True) for k, v in p.items()}
    with torch.enable_grad():
        out = oracle_render(shape, api, q, dt)
    return q, out


def oracle_outputs(shape: str, api: str, dt):
    return {k: v.detach() for k, v in _oracle_forward(shape, api, dt)[1].items()}


# ---------------------------------------------------------------------------------------------------------------------
# the weight_max selection and the cotangents
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weight_max_selection(shape: str):
    """(kept [B] bool, fp64 arg-max [B], margin): the rays whose fp64 top-two weight gap exceeds
    margin = 2 x parity.value_bound(w64, max|w32 - w64|).  (The weights do not depend on lights or background: any api.)"""
    w64 = oracle_outputs(shape, "render_rnb", torch.float64)["weights"]
    w32 = oracle_outputs(shape, "render_rnb", torch.float32)["weights"]
    margin = 2.0 * P.value_bound(w64, P.max_err(w32, w64))
    top = torch.topk(w64, 2, dim=-1)
    kept = (top.values[:, 0] - top.values[:, 1]) > margin
    return kept, top.indices[:, 0], margin


def _out_shapes(shape: str, api: str):
    B = RAYS[shape][0]
    L = batch(shape, api)["lights_dir"].shape[0]
    return {"color_fine": (B, 3) if api == "render" else (L, B, 3), "s_val": (B, 1), "cdf_fine": (B, S), "weight_sum": (B, 1),
            "weight_max": (B, 1), "gradients": (B, S, 3), "weights": (B, S), "gradient_error": ()}


@functools.lru_cache(maxsize=None)
def cotangents(shape: str, api: str):
    """{output: fp64 cotangent}: randn / sqrt(numel) from one generator over FLOAT_OUTS; weight_max's is zero on the rays
    weight_max_selection drops.  Shared (never written) by every row of (shape, api)."""
    g = torch.Generator().manual_seed(COT_SEED)
    shapes = _out_shapes(shape, api)
    cot = {}
    for k in FLOAT_OUTS:
        n = 1
        for d in shapes[k]:
            n *= d
        cot[k] = torch.randn(shapes[k], generator=g, dtype=torch.float64) / max(1, n) ** 0.5
    kept, _, _ = weight_max_selection(shape)
    cot["weight_max"] = cot["weight_max"] * kept[:, None].to(torch.float64)
    return cot


def functional(row: AdjRow, out):
    """sum over the row's outputs of (cotangent . output), in the outputs' dtype and on their device"""
    cot = cotangents(row.shape, row.api)
    total = 0.0
    for k in row.outputs:
        t = out[k]
        assert tuple(t.shape) == tuple(cot[k].shape), f"{row.name}: {k} has shape {tuple(t.shape)}"
        total = total + (cot[k].to(t.device, t.dtype) * t).sum()
    return total


def oracle_grads(row: AdjRow, dt):
    """{leaf: d functional / d leaf, or None where autograd finds no path} of the oracle in dtype dt"""
    q, out = _oracle_forward(row.shape, row.api, dt)
    names = list(q)
    with torch.enable_grad():
        gs = torch.autograd.grad(functional(row, out), [q[k] for k in names], retain_graph=True, allow_unused=True)
    return dict(zip(names, gs))


def is_zero(g) -> bool:
    return g is None or not bool((g != 0).any())


# ---------------------------------------------------------------------------------------------------------------------
# the variance clip: inv_s = exp(10 variance).clip(1e-6, 1e6)
# ---------------------------------------------------------------------------------------------------------------------
# +-1.3815: raw inv_s 9.995e5 / 1.0005e-6, just inside; +-1.4: 1.2e6 / 8.3e-7, outside
CLIP_VARIANCES = ((1.3815, True), (-1.3815, True), (1.4, False), (-1.4, False))
CLIP_SHAPE, CLIP_API = "w32", "render_rnb"


def clip_params(variance: float):
    _, p = model(CLIP_SHAPE)
    q = dict(p)
    q[VARIANCE] = torch.tensor(float(variance))
    return q


def clip_loss(out, b):
    """the training loss plus sum(s_val): the s_val term gives d loss / d variance a part that does not pass the weights"""
    return O.rnb_loss(out, b["true_rgb"], b["mask"])[0] + out["s_val"].sum()


def clip_oracle(variance: float, dt):
    """(outputs, {leaf: gradient}) of the oracle at dev.variance = variance"""
    q = {k: v.detach().to(dt).requires_grad_(True) for k, v in clip_params(variance).items()}
    b = {k: v.to(dt) for k, v in batch(CLIP_SHAPE, CLIP_API).items()}
    with torch.enable_grad():
        out = oracle_render(CLIP_SHAPE, CLIP_API, q, dt)
        clip_loss(out, b).backward()
    return {k: v.detach() for k, v in out.items()}, {k: v.grad for k, v in q.items()}
