"""The mesh extraction chain of `NeuSRenderer.extract_geometry` / `extract_textured_geometry`, written once: the volume
(dense or sparse), marching cubes, the mesh stages in the order of `STAGES`, and the rescaling from grid-index units to
the bounding box.  A new mesh stage is one more row of `STAGES`; nothing in renderer.py names a stage."""
from __future__ import annotations

from functools import partial
from typing import Callable, NamedTuple, Optional

import torch

from . import mesh_clean, mesh_cull, mesh_fill, mesh_simplify, native, texture_bake
from .mcubes import marching_cubes


def rescale_to_bounds_host(vertices, bound_min, bound_max, res):
    """Grid-index vertices (numpy [V,3] float64) to the bounding box: models/renderer.py:34-35, the reference's
    expression in numpy.  `rescale_to_bounds_device` is this function bit for bit (tests/test_mesh_pipeline_host.py): the
    two are the only places that hold the expression."""
    b_max, b_min = bound_max.detach().cpu().numpy(), bound_min.detach().cpu().numpy()
    return vertices / (res - 1.0) * (b_max - b_min)[None, :] + b_min[None, :]


def rescale_to_bounds_device(vertices, bound_min, bound_max, res):
    """`rescale_to_bounds_host` on the tensor's device, bit for bit: float64, the box's extent taken in the bounds' own
    precision first and then widened; an element-wise division (a division by a Python scalar is a multiplication by its
    reciprocal there)."""
    b_min, b_max = (b.detach().to(vertices.device) for b in (bound_min, bound_max))
    return (vertices / torch.full_like(vertices, float(res) - 1.0) * (b_max - b_min).double()[None, :]
            + b_min.double()[None, :])


def grid_desc(bound_min, bound_max, res, x_begin, x_end):
    """The `rnb_grid_desc` of the x-planes [x_begin, x_end) of a res^3 grid over the box, values negated (out_scale -1)"""
    gd = native.GridDesc()
    for d in range(3):
        gd.bound_min[d] = float(bound_min[d])
        gd.bound_max[d] = float(bound_max[d])
    gd.resolution, gd.x_begin, gd.x_end, gd.out_scale = res, x_begin, x_end, -1.0
    return gd


def cell_diagonal(bound_min, bound_max, res):
    """One cell diagonal of the res^3 grid over the box, in model units: the default `max_step` of a refinement"""
    return sum(((float(bound_max[d]) - float(bound_min[d])) / (res - 1)) ** 2 for d in range(3)) ** 0.5


# ------------------------------------------------------------------------------------------------------------ the stages
# run(v, t, options, frame) -> (v, t, info): device (v, t) in grid-index units in and out; frame = (bound_min, bound_max, res)
def _clean(v, t, options, frame):
    out = mesh_clean.clean_mesh(v, t, **options)
    return out["vertices"], out["triangles"], out["info"]


def _cull(v, t, options, frame):
    """the votes are taken in the cameras' frame, on the rescaled vertices; the survivors come back in grid-index units"""
    out = mesh_cull.cull_mesh(rescale_to_bounds_device(v, *frame), t, **options)
    return v.index_select(0, out["vertex_index"]), out["triangles"], out["info"]


def _simplify(v, t, options, frame):
    out = mesh_simplify.simplify_mesh(v, t, **options)
    return out["vertices"], out["triangles"], out["info"]


class Stage(NamedTuple):
    """One option of the extract calls that is a dict of another function's keywords.  `said`: how the error message names
    those keywords (the two older options list them bare, the two newer ones as the tuple prints: kept as they were)."""
    name: str
    keywords: tuple
    check: Callable                 # check(name, **options): ValueError for options that cannot work
    said: str
    run: Optional[Callable] = None
    info: Optional[str] = None      # the renderer attribute that receives the stage's `info`


STAGES = (
    Stage("clean", mesh_clean.CLEAN_KEYWORDS, partial(mesh_clean.check_criteria, has_vertices=True),
          f"clean_mesh keywords ({', '.join(mesh_clean.CLEAN_KEYWORDS)})", _clean, "last_mesh_clean"),
    Stage("cull", mesh_cull.CULL_KEYWORDS, mesh_cull.check_arguments,
          f"cull_mesh keywords {mesh_cull.CULL_KEYWORDS}", _cull, "last_mesh_cull"),
    Stage("simplify", mesh_simplify.SIMPLIFY_KEYWORDS, mesh_simplify.check_arguments,
          f"simplify_mesh keywords ({', '.join(mesh_simplify.SIMPLIFY_KEYWORDS)})", _simplify, "last_mesh_simplify"),
)
# `bake=` of the textured call is checked like a stage's options and is not a stage: it runs on the final, rescaled mesh
BAKE = Stage("bake", texture_bake.BAKE_KEYWORDS, partial(texture_bake.check_arguments, need_max_step=False),
             f"bake_textures keywords {texture_bake.BAKE_KEYWORDS}")
# `fill=` closes the holes the stages leave: checked like a stage's options, run after the last stage and before the rescale
# (`run_fill`), and not a row of `STAGES`, whose order and length an existing test holds fixed
FILL = Stage("fill", mesh_fill.FILL_KEYWORDS, mesh_fill.check_arguments,
             f"fill_holes keywords {mesh_fill.FILL_KEYWORDS}", info="last_mesh_fill")
_OPTIONS = {s.name: s for s in STAGES + (BAKE, FILL)}


def check_options(**options):
    """The `clean`, `cull`, `simplify`, `bake` and `fill` arguments of the extract calls, in the order given and before any grid
    is evaluated: None, or a dict whose keys are the option's keywords and which its module's checker accepts."""
    for name, value in options.items():
        if value is None:
            continue
        opt = _OPTIONS[name]
        if not isinstance(value, dict) or not set(value) <= set(opt.keywords):
            raise ValueError(f"{name} must be a dict of {opt.said}")
        opt.check(name, **value)


def run_stages(renderer, v, t, frame, options):
    """The stages `options` asks for ({name: dict or None}), in the order of `STAGES`, on device (v, t) in grid-index
    units; every stage that ran leaves its `info` on the renderer."""
    for stage in STAGES:
        if options.get(stage.name) is not None:
            v, t, info = stage.run(v, t, options[stage.name], frame)
            setattr(renderer, stage.info, info)
    return v, t


def run_fill(renderer, v, t, fill):
    """`fill_holes(v, t, **fill)` on device (v, t) in grid-index units when `fill` is a dict, its `info` left on the renderer;
    (v, t) as they are for None"""
    if fill is None:
        return v, t
    out = mesh_fill.fill_holes(v, t, **fill)
    setattr(renderer, FILL.info, out["info"])
    return out["vertices"], out["triangles"]


# ------------------------------------------------------------------------------------------------------------- the chain
def volume(renderer, bound_min, bound_max, res, threshold, sparse, brick, margin, to_host):
    """The SDF grid of the chain: `extract_fields`, or with `sparse` `extract_fields_sparse` (its `info` kept in
    `renderer.last_sparse_grid`)"""
    if sparse:
        u, renderer.last_sparse_grid = renderer.extract_fields_sparse(bound_min, bound_max, res, threshold, brick, margin,
                                                                      to_host=to_host)
        return u
    return renderer.extract_fields(bound_min, bound_max, res, to_host=to_host)


def device_mesh(renderer, bound_min, bound_max, res, threshold, sparse, brick, margin, options, fill=None):
    """Volume, native marching cubes, the stages and the hole filling without leaving the device: (v, t) in grid-index
    units.  The volume is released before the first stage."""
    u = volume(renderer, bound_min, bound_max, res, threshold, sparse, brick, margin, to_host=False)
    v, t = marching_cubes(u, threshold)
    del u
    return run_fill(renderer, *run_stages(renderer, v, t, (bound_min, bound_max, res), options), fill)
