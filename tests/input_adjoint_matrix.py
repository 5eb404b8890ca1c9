"""The gradients of a render with respect to its INPUTS (rnb_render_input_grads: rays_o, rays_d, lights_dir, background_rgb,
z_vals) under each cotangent of the render alone: the table of tests/adjoint_matrix.py, which is reused unchanged (rows,
model, batch, depths at S = 80, cotangents, functional, weight_max selection; 16 rays on w32, 64 on default_64x64), with
the inputs as the leaves and a few rows more.

A plain module: tests/test_input_adjoint_matrix_host.py pins it on the CPU oracle (the declared zeros are the oracle's
zeros, every other (row, input) is a parity target the fp32 oracle resolves), tests/test_gpu_input_adjoint_matrix.py runs
it on the device.

Why one cotangent at a time.  Every other device-vs-fp64 comparison of an input gradient drives all eight outputs and the
training loss together and judges the whole tensor by rel-L2.  The norm of z_vals.grad on default_64x64 / render_rnb is
6.4 under "all", 2.8 under weights, 2.2 under cdf_fine and 1.2 under gradients, but 1.3e-2 under color_fine, 9.3e-3 under
weight_sum and 6.0e-3 under gradient_error: a 5 % error in how one of the last three reaches z_vals moves the combined
gradient by less than the 1e-4 floor of parity.grad_bound.

Rows: adjoint_matrix.ROWS, and for the inputs only
  default_64x64 x render_rnb_no_albedo x {color_fine, weights, gradients, gradient_error, all}
                (no albedo network in the call: ray_input_adjoint_kernel gets no cinb, its `else { pb = 0 }` branch)
  default_64x64 x render_rnb_warmup    x {color_fine, gradients, all}      (shared lights [L,1,1,3]: sum_over_rays_kernel)
  default_64x64 x render               x all
  w32           x render_rnb_no_albedo x {gradients, weight_sum, all}

Inputs per api (INPUTS): render has rays_o, rays_d, z_vals, background_rgb; every render_rnb* api has rays_o, rays_d,
z_vals, lights_dir.  near / far do not enter a render at explicit depths.

The oracle runs with the graph-keeping normal of tests/oracle_normal.py (the normal's Hessian-vector term is part of the
reference's ray gradient), one forward per (shape, api, dtype) with the inputs as leaves, shared by every adjoint of it.

Structural zeros, by name, held to exactly 0.0 on the device (a rel-L2 rule divides by zero there):
  every input under s_val (s_val = 1 / inv_s);
  lights_dir and background_rgb under every adjoint except color_fine and "all" (only the colour reads them);
  under weight_max the rows of rays_o, rays_d and z_vals that belong to the rays adjoint_matrix.weight_max_selection
  drops (1 of 16 on w32, 11 of 64 on default_64x64: their cotangent is zero and a ray's outputs depend on that ray's
  inputs alone); the kept rays' rows go by the gradient rule.

The rule is parity.check_grad per WHOLE tensor: rays_o [B,3], rays_d [B,3], z_vals [B,S], lights_dir, background_rgb [3].
Never per ray: on the CPU oracle the fp32 run is already 100 % off on single rays that miss the surface, whose rows are
1e-8 of the tensor's norm; a per-ray rel-L2 would refuse those rows for the reference's own arithmetic."""
from __future__ import annotations

import functools

import torch

from oracle import rnb_oracle as O
from tests import adjoint_matrix as M
from tests.oracle_normal import graph_normal_installed

AdjRow = M.AdjRow

EXTRA_ROWS = (
    [AdjRow("default_64x64", "render_rnb_no_albedo", adj) for adj in ("color_fine", "weights", "gradients", "gradient_error", "all")]
    + [AdjRow("default_64x64", "render_rnb_warmup", adj) for adj in ("color_fine", "gradients", "all")]
    + [AdjRow("default_64x64", "render", "all")]
    + [AdjRow("w32", "render_rnb_no_albedo", adj) for adj in ("gradients", "weight_sum", "all")]
)
INPUT_ROWS = list(M.ROWS) + EXTRA_ROWS
BY_NAME = {r.name: r for r in INPUT_ROWS}
assert len(BY_NAME) == len(INPUT_ROWS), "row names must be unique"

RAY_INPUTS = ("rays_o", "rays_d", "z_vals")
INPUTS = {
    "render": RAY_INPUTS + ("background_rgb",),
    "render_rnb": RAY_INPUTS + ("lights_dir",),
    "render_rnb_warmup": RAY_INPUTS + ("lights_dir",),
    "render_rnb_no_albedo": RAY_INPUTS + ("lights_dir",),
}
assert set(INPUTS) == set(M.APIS)

# ---------------------------------------------------------------------------------------------------------------------
# the inputs no cotangent of the row reaches, by name
# ---------------------------------------------------------------------------------------------------------------------
_COLOUR_ONLY = frozenset(("lights_dir", "background_rgb"))
_EVERY_INPUT = frozenset(RAY_INPUTS) | _COLOUR_ONLY
ZERO_INPUTS = {
    "color_fine": frozenset(),
    "weights": _COLOUR_ONLY,
    "cdf_fine": _COLOUR_ONLY,
    "gradients": _COLOUR_ONLY,
    "weight_sum": _COLOUR_ONLY,
    "weight_max": _COLOUR_ONLY,
    "gradient_error": _COLOUR_ONLY,
    "s_val": _EVERY_INPUT,
    "all": frozenset(),
}
assert set(ZERO_INPUTS) == set(M.ADJOINTS) | {"all"}


def inputs(row: AdjRow):
    return INPUTS[row.api]


def zero_inputs(row: AdjRow):
    """the inputs of the row's api whose whole gradient is zero"""
    return ZERO_INPUTS[row.adjoint] & frozenset(INPUTS[row.api])


def zero_rays(row: AdjRow):
    """[B] bool: the rays whose rows of rays_o / rays_d / z_vals are zero while the others are live (weight_max: the rays
    its selection drops), or None where every ray is live"""
    if row.adjoint != "weight_max":
        return None
    kept, _, _ = M.weight_max_selection(row.shape)
    return ~kept


# ---------------------------------------------------------------------------------------------------------------------
# the oracle with the inputs as leaves
# ---------------------------------------------------------------------------------------------------------------------
def input_values(shape: str, api: str, shared_lights=None):
    """{input: fp32 CPU tensor} of an api at the table's batch and depths: what the device and both oracles are handed.
    `shared_lights`: None for the table's lights (per ray [L,B,1,3], the warm-up's shared [L,1,1,3]); True / False force the
    warm-up batch's shared lights / render_rnb's per-ray ones onto any render_rnb* api."""
    b = M.batch(shape, api)
    x = {"rays_o": b["rays_o"], "rays_d": b["rays_d"], "z_vals": M.depths(shape)}
    if api == "render":
        assert shared_lights is None
        x["background_rgb"] = torch.tensor(M.BACKGROUND)
    elif shared_lights is None:
        x["lights_dir"] = b["lights_dir"]
    else:
        x["lights_dir"] = M.batch(shape, "render_rnb_warmup" if shared_lights else "render_rnb")["lights_dir"]
    assert set(x) == set(INPUTS[api])
    return x


def oracle_render(shape: str, api: str, q, x):
    """the oracle's render of `api` with the parameters q and the inputs x (both already of the oracle's dtype), under the
    graph-keeping normal"""
    mc, _ = M.model(shape)
    dt = x["rays_o"].dtype
    b = {k: v.to(dt) for k, v in M.batch(shape, api).items()}
    with graph_normal_installed():
        if api == "render":
            return O.render(q, mc, x["rays_o"], x["rays_d"], b["near"], b["far"], background_rgb=x["background_rgb"],
                            cos_anneal_ratio=M.COS_ANNEAL, z_vals=x["z_vals"])
        return O.render_rnb(q, mc, x["rays_o"], x["rays_d"], b["near"], b["far"], x["lights_dir"], cos_anneal_ratio=M.COS_ANNEAL,
                            warmup=api == "render_rnb_warmup", no_albedo=api == "render_rnb_no_albedo", z_vals=x["z_vals"])


@functools.lru_cache(maxsize=None)
def _oracle_forward(shape: str, api: str, dt, shared_lights=None):
    """(input leaves, outputs with their graph): one forward per (shape, api, dtype), shared by every adjoint of it"""
    _, p = M.model(shape)
    q = {k: v.detach().to(dt) for k, v in p.items()}
    x = {k: v.detach().to(dt).requires_grad_(True) for k, v in input_values(shape, api, shared_lights).items()}
    with torch.enable_grad():
        out = oracle_render(shape, api, q, x)
    return x, out


def oracle_outputs(shape: str, api: str, dt, shared_lights=None):
    return {k: v.detach() for k, v in _oracle_forward(shape, api, dt, shared_lights)[1].items()}


def oracle_input_grads(row: AdjRow, dt, shared_lights=None):
    """{input: d functional / d input, or None where autograd finds no path} of the oracle in dtype dt"""
    x, out = _oracle_forward(row.shape, row.api, dt, shared_lights)
    names = list(INPUTS[row.api])
    with torch.enable_grad():
        f = M.functional(row, out)
        if not f.requires_grad:      # s_val: a function of the variance alone
            return {k: None for k in names}
        gs = torch.autograd.grad(f, [x[k] for k in names], retain_graph=True, allow_unused=True)
    return dict(zip(names, gs))


is_zero = M.is_zero
