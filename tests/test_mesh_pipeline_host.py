"""Host side of the extraction chain (rnb_neus_fork_amd.mesh_pipeline, mesh_args, native.workspace): the two rescales are
the expressions they replaced bit for bit, every option of the extract calls is checked with the messages it always had
and before a grid is evaluated, the stage table has its order, the workspace helper reaches every size query, and the
merged box of the finite vertices is both boxes it replaced.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import rnb_neus_fork_amd as R
from rnb_neus_fork_amd import mesh_args as A
from rnb_neus_fork_amd import mesh_pipeline as P
from tests import mesh_attrs_util as U

N = R.native
BOXES = {"cube": (U.LO, U.HI),
         "asymmetric": (torch.tensor([-0.3, -1.7, 0.25]), torch.tensor([1.1, 0.9, 2.6]))}     # float32, unequal sides


def _grid_vertices(res):
    """[64,3] float64 in grid-index units: 0, res - 1, non-terminating binary fractions, a negative value, random rows"""
    g = torch.Generator().manual_seed(res)
    v = torch.rand(64, 3, generator=g, dtype=torch.float64) * (res - 1)
    v[0] = 0.0
    v[1] = res - 1.0
    v[2] = torch.tensor([0.1, (res - 1) / 3.0, 0.7 * (res - 1)], dtype=torch.float64)
    v[3] = torch.tensor([-0.3, 1.0 / 3.0, (res - 1) - 0.1], dtype=torch.float64)
    return v


@pytest.mark.parametrize("box", sorted(BOXES))
@pytest.mark.parametrize("res", [2, 40, 513])
def test_the_two_rescales_are_the_expressions_they_replaced_bit_for_bit(res, box):
    bound_min, bound_max = BOXES[box]
    assert bound_min.dtype == torch.float32
    v = _grid_vertices(res)
    host = P.rescale_to_bounds_host(v.numpy(), bound_min, bound_max, res)
    dev = P.rescale_to_bounds_device(v, bound_min, bound_max, res)
    assert host.dtype == np.float64 and dev.dtype == torch.float64 and host.shape == (64, 3) == tuple(dev.shape)
    assert np.array_equal(host.view(np.uint64), dev.numpy().view(np.uint64)), "device and host rescale differ"
    assert torch.equal(torch.from_numpy(host).view(torch.int64), dev.view(torch.int64))
    # the parent's inline expressions, literally: extract_geometry / extract_textured_geometry(to_host=True) ...
    vertices, resolution = v.numpy(), res
    b_max, b_min = bound_max.detach().cpu().numpy(), bound_min.detach().cpu().numpy()
    want = vertices / (resolution - 1.0) * (b_max - b_min)[None, :] + b_min[None, :]
    assert np.array_equal(host.view(np.uint64), want.view(np.uint64))
    # ... extract_textured_geometry(to_host=False) ...
    b_min, b_max = (b.detach().to(v.device) for b in (bound_min, bound_max))
    want = v / torch.full_like(v, res - 1.0) * (b_max - b_min).double()[None, :] + b_min.double()[None, :]
    assert torch.equal(dev.view(torch.int64), want.view(torch.int64))
    # ... and the cull's
    want = v / torch.full_like(v, float(resolution) - 1.0) * (b_max - b_min).double()[None, :] + b_min.double()[None, :]
    assert torch.equal(dev.view(torch.int64), want.view(torch.int64))
    assert host[0].tolist() == [float(x) for x in bound_min] and not np.array_equal(host[1], host[0])


def test_cell_diagonal_and_grid_desc():
    lo, hi = BOXES["asymmetric"]
    for res in (2, 40):
        want = sum(((float(hi[d]) - float(lo[d])) / (res - 1)) ** 2 for d in range(3)) ** 0.5
        assert P.cell_diagonal(lo, hi, res) == want == P.cell_diagonal([float(x) for x in lo], [float(x) for x in hi], res)
    gd = P.grid_desc(lo, hi, 40, 3, 17)
    assert list(gd.bound_min) == [float(x) for x in lo] and list(gd.bound_max) == [float(x) for x in hi]
    assert (gd.resolution, gd.x_begin, gd.x_end, gd.out_scale) == (40, 3, 17, -1.0)


def test_the_stage_table():
    assert tuple(s.name for s in P.STAGES) == ("clean", "cull", "simplify")
    assert tuple(s.info for s in P.STAGES) == ("last_mesh_clean", "last_mesh_cull", "last_mesh_simplify")
    assert [s.keywords for s in P.STAGES] == [R.mesh_clean.CLEAN_KEYWORDS, R.mesh_cull.CULL_KEYWORDS,
                                              R.mesh_simplify.SIMPLIFY_KEYWORDS]
    assert all(callable(s.run) and callable(s.check) for s in P.STAGES)
    assert P.BAKE not in P.STAGES and P.BAKE.run is None and P.BAKE.keywords == R.texture_bake.BAKE_KEYWORDS


_CAMERAS = {"projections": torch.zeros(1, 3, 4, dtype=torch.float64), "eyes": torch.zeros(1, 3, dtype=torch.float64)}
# option -> (a non-dict, an unknown key: both get the first message), (a bad value, its message)
MESSAGES = {
    "clean": ("clean must be a dict of clean_mesh keywords (by, keep_largest, min_fraction, min_triangles)",
              ("largest", {"keep": 1}, {"attributes": {}}),
              ({"keep_largest": 0}, "clean: keep_largest must be an integer >= 1, not 0")),
    "cull": ("cull must be a dict of cull_mesh keywords ('rays', 'views', 'projections', 'eyes', 'masks', 'image_size', "
             "'max_outside', 'min_seen', 'occlusion', 'dilate', 'threshold', 'rule')",
             ([1], dict(_CAMERAS, index=None), dict(_CAMERAS, attributes={})),
             (dict(_CAMERAS, image_size=(4, 4), rule="some"), "cull: rule must be one of ('all', 'any'), not 'some'")),
    "simplify": ("simplify must be a dict of simplify_mesh keywords (cell_size, target_triangles, origin)",
                 ("small", {"cells": 2}, {"cell_size": 2.0, "attributes": {}}),
                 ({"cell_size": 0.0}, "simplify: cell_size must be a positive finite number, not 0.0")),
    "bake": ("bake must be a dict of bake_textures keywords ('size', 'chart', 'refine', 'max_step', 'threshold', 'albedo', "
             "'slab', 'chunk', 'return_samples')",
             ("yes", {"charts": 4}, {"to_host": False}),
             ({"chart": 0}, "bake: chart must be an integer >= 1 and <= 255, not 0")),
}
GOOD = {"clean": {"keep_largest": 1}, "cull": dict(_CAMERAS, image_size=(4, 4)), "simplify": {"cell_size": 2.0},
        "bake": {"chart": 4}}


@pytest.fixture(scope="module")
def cpu_renderer():
    mc, p, _ = U.model("tiny")
    return R.build_from_named_params(mc, p, torch.device("cpu"))[3]


@pytest.mark.parametrize("option", sorted(MESSAGES))
def test_every_option_is_checked_with_its_message_before_any_grid(cpu_renderer, option):
    ren = cpu_renderer
    not_keywords, shapes, (bad_value, bad_message) = MESSAGES[option]
    calls = [lambda **kw: ren.extract_textured_geometry(U.LO, U.HI, 8, **kw)]
    if option != "bake":        # (an option of the textured call only)
        calls.append(lambda **kw: ren.extract_geometry(U.LO, U.HI, 8, backend="native", **kw))
    for call in calls:
        for bad in shapes:
            with pytest.raises(ValueError) as e:
                call(**{option: bad})
            assert str(e.value) == not_keywords
        with pytest.raises(ValueError) as e:
            call(**{option: bad_value})
        assert str(e.value) == bad_message
        # options that pass reach the grid, which a CPU renderer cannot evaluate (the dense grid stops at packing the
        # weights, the sparse one at its device check): the ValueErrors above came before it
        for value in (GOOD[option], None):
            with pytest.raises(AssertionError, match="on the GPU"):
                call(**{option: value})
            with pytest.raises(RuntimeError, match="GPU tensors only"):
                call(sparse=True, **{option: value})
    P.check_options(**{option: None})
    P.check_options(**{option: GOOD[option]})
    with pytest.raises(ValueError) as e:
        P.check_options(**{option: bad_value})
    assert str(e.value) == bad_message


def test_options_are_checked_in_the_order_given(cpu_renderer):
    """the first failing check of a call with several bad options is the one it always was: clean, simplify, (bake,) cull"""
    bad = {k: MESSAGES[k][2][0] for k in MESSAGES}
    with pytest.raises(ValueError, match="^simplify: "):
        cpu_renderer.extract_geometry(U.LO, U.HI, 8, backend="native", simplify=bad["simplify"], cull=bad["cull"])
    with pytest.raises(ValueError, match="^clean: "):
        cpu_renderer.extract_geometry(U.LO, U.HI, 8, backend="native", cull=bad["cull"], clean=bad["clean"])
    with pytest.raises(ValueError, match="^bake: "):
        cpu_renderer.extract_textured_geometry(U.LO, U.HI, 8, cull=bad["cull"], bake=bad["bake"])
    with pytest.raises(ValueError, match="^simplify: "):
        cpu_renderer.extract_textured_geometry(U.LO, U.HI, 8, bake=bad["bake"], simplify=bad["simplify"])


def _size_arguments(desc):
    gd = P.grid_desc(U.LO, U.HI, 20, 0, 20)
    sd = N.SparseGridDesc(8, 0.0, 1.0)
    d = C.byref(desc)
    return {"points": (d, 1000), "points_grad": (d, 1000, N.POINTS_FEATURE), "sdf_grid": (d, C.byref(gd)),
            "sdf_grid_sparse": (d, C.byref(gd), C.byref(sd)), "marching_cubes": (20, 21, 22),
            "mesh_vertex": (d, 4096, N.MESH_ALBEDO), "mesh_clean": (1000, 2000), "mesh_simplify": (1000, 2000),
            "mesh_bins": (4096,), "mesh_sample": (2000,), "sample": (d, 64), "render": (d, 64, 32, N.MODE_MVPS)}


def test_workspace_reaches_every_size_query_and_applies_the_floor(cpu_renderer):
    args = _size_arguments(cpu_renderer.desc)
    queries = sorted(s for s in N._SIGNATURES if s.endswith("_workspace_bytes"))
    assert sorted(f"rnb_{name}_workspace_bytes" for name in args) == queries
    lib = N.load()
    for name, a in args.items():
        need = C.c_int64(-1)
        N.check(getattr(lib, f"rnb_{name}_workspace_bytes")(*a, C.byref(need)))
        assert need.value >= 0, name
        assert N.workspace_bytes(name, *a) == need.value and N.workspace_bytes(name, *a, floor=need.value + 3) == need.value + 3
        ws = N.workspace(name, "cpu", *a)
        assert ws.dtype == torch.uint8 and ws.dim() == 1 and ws.numel() == need.value, name
        assert N.workspace(name, "cpu", *a, floor=need.value + 17).numel() == need.value + 17, name
        assert N.workspace(name, "cpu", *a, floor=max(need.value - 1, 0)).numel() == need.value, name
    with pytest.raises(AttributeError):
        N.workspace("no_such_call", "cpu", 1)
    with pytest.raises(N.NativeError):      # the return code is checked
        N.workspace("mesh_bins", "cpu", -7)


def _box_of_mesh_index(vertices):
    """the parent's MeshIndex.__init__, literally, with its host step: (lo, hi) as lists"""
    V = vertices.shape[0]
    box = torch.zeros(2, 3, dtype=torch.float64)
    if V > 0:
        fin = torch.isfinite(vertices).all(dim=1, keepdim=True)
        big = torch.finfo(torch.float64).max
        lo = torch.where(fin, vertices, torch.full_like(vertices, big)).min(dim=0).values
        hi = torch.where(fin, vertices, torch.full_like(vertices, -big)).max(dim=0).values
        box = torch.stack([lo, hi])
    lo, hi = box[0].tolist(), box[1].tolist()
    if any(h < l for l, h in zip(lo, hi)):        # no finite vertex
        lo, hi = [0.0] * 3, [0.0] * 3
    return lo, hi


def _box_of_simplify(vts):
    """the parent's mesh_simplify._finite_box, literally"""
    ok = torch.isfinite(vts).all(dim=1, keepdim=True)
    inf = torch.full_like(vts, float("inf"))
    lo = torch.where(ok, vts, inf).amin(dim=0) if vts.shape[0] else inf.new_full((3,), float("inf"))
    hi = torch.where(ok, vts, -inf).amax(dim=0) if vts.shape[0] else inf.new_full((3,), float("-inf"))
    none = torch.isinf(lo)
    return torch.where(none, torch.zeros_like(lo), lo), torch.where(none, torch.zeros_like(hi), hi)


def test_finite_box_is_both_boxes_it_replaced():
    big, nan, inf = torch.finfo(torch.float64).max, float("nan"), float("inf")
    g = torch.Generator().manual_seed(4)
    cloud = torch.randn(257, 3, generator=g, dtype=torch.float64)
    holes = cloud.clone()
    holes[5, 1], holes[77, 0], holes[200, 2] = nan, inf, -inf
    holes[int(cloud[:, 0].argmin())] = nan      # the vertex that held an extreme is one of the dropped ones
    cases = {"V = 0": torch.zeros(0, 3, dtype=torch.float64),
             "no finite vertex": torch.tensor([[nan, 0.0, 0.0], [1.0, inf, 2.0], [0.0, 0.0, -inf]], dtype=torch.float64),
             "one vertex": torch.tensor([[1.5, -2.5, 0.25]], dtype=torch.float64),
             "+max": torch.tensor([[big, big, big]], dtype=torch.float64),
             "-max": torch.tensor([[-big, -big, -big]], dtype=torch.float64),
             "both max": torch.tensor([[big, -big, 0.0], [-big, big, 1.0], [nan, nan, nan]], dtype=torch.float64),
             "max beside a hole": torch.tensor([[big, 1.0, -big], [inf, -big, big], [2.0, 3.0, 4.0]], dtype=torch.float64),
             "cloud": cloud, "cloud with holes": holes}
    for tag, v in cases.items():
        lo, hi = A.finite_box(v)
        assert lo.shape == hi.shape == (3,) and lo.dtype == hi.dtype == torch.float64, tag
        s_lo, s_hi = _box_of_simplify(v)
        assert torch.equal(lo, s_lo) and torch.equal(hi, s_hi), tag
        m_lo, m_hi = _box_of_mesh_index(v)
        assert lo.tolist() == m_lo and hi.tolist() == m_hi, tag
    assert A.finite_box(cases["no finite vertex"])[0].tolist() == [0.0] * 3 == A.finite_box(cases["V = 0"])[1].tolist()
    assert A.finite_box(cases["max beside a hole"])[1].tolist() == [big, 3.0, 4.0]


def test_no_module_reaches_into_a_sibling():
    import glob
    import os
    import re
    pkg = os.path.dirname(os.path.abspath(R.__file__))
    said = 0
    for path in sorted(glob.glob(os.path.join(pkg, "*.py"))):
        text = open(path).read()
        assert not re.search(r"^\s*from \.\w+ import .*\b_[a-z]", text, re.M), path
        said += text.count("works on GPU tensors only")
    assert said == 1, "the no-CPU-path sentence is native.NO_CPU_PATH and is spelled out there alone"
