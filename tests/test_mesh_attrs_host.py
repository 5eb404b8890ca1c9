"""Host side of the per-vertex mesh attributes (rnb_mesh_vertex_workspace_bytes / rnb_mesh_vertex_attrs): the symbols are
declared, bound and exported together, the workspace query is a host function of the chunk size alone, and the argument
checks that come before any launch.  No GPU."""
import ctypes as C
import os
import re

import pytest
import torch

import rnb_neus_fork_amd as R
from tests import mesh_attrs_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rnb_mesh_vertex_workspace_bytes", "rnb_mesh_vertex_attrs")


def _desc(which="tiny", variant=0):
    mc, p, _ = U.model(which)
    ren = R.build_from_named_params(mc, p, torch.device("cpu"))[3]
    ren.desc.variant = variant
    return ren.desc


def _ws_bytes(desc, chunk, flags):
    b = C.c_int64(-7)
    return R.native.load().rnb_mesh_vertex_workspace_bytes(C.byref(desc), chunk, flags, C.byref(b)), b.value


def test_symbols_are_declared_bound_and_exported():
    lib = R.native.load()
    header = open(os.path.join(ROOT, "include", "rnbneus.h")).read()
    for name in SYMBOLS:
        assert name in R.native.EXPORTED_SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/rnbneus.h"
        assert hasattr(lib, name)
    assert "typedef struct rnb_mesh_vertex_args" in header
    assert lib.rnb_abi_version() == 5 and R.native.ABI_VERSION == 5
    # the binding's structure is the header's: field order and the 64-bit count behind two pointers
    names = [f[0] for f in R.native.MeshVertexArgs._fields_]
    decl = header.split("typedef struct rnb_mesh_vertex_args {")[1].split("} rnb_mesh_vertex_args;")[0]
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    declared = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", decl)
    assert names == declared
    assert R.native.MeshVertexArgs.V.offset == 16 and R.native.MESH_ALBEDO == 1 and R.native.MESH_SWAP_RB == 2


@pytest.mark.parametrize("which,variant", [("tiny", 0), ("sharp", 0), ("sharp", R.native.VARIANT_BF16)])
def test_workspace_covers_the_point_state_and_depends_on_the_chunk_alone(which, variant):
    lib = R.native.load()
    desc = _desc(which, variant)
    pts = C.c_int64()
    R.native.check(lib.rnb_points_workspace_bytes(C.byref(desc), 4096, C.byref(pts)))
    seen = set()
    for flags in (0, R.native.MESH_ALBEDO, R.native.MESH_ALBEDO | R.native.MESH_SWAP_RB):
        rc, b = _ws_bytes(desc, 4096, flags)
        assert rc == 0 and b >= pts.value + 4096 * 3 * 4      # the point state + the chunk's point buffer
        seen.add(b)
    # no vertex count enters the query: the size is a function of the chunk (and grows with it)
    rc, small = _ws_bytes(desc, 64, R.native.MESH_ALBEDO)
    rc2, large = _ws_bytes(desc, 8192, R.native.MESH_ALBEDO)
    assert rc == 0 and rc2 == 0 and small < min(seen) <= max(seen) < large


def test_bad_chunks_and_flags_are_refused():
    lib = R.native.load()
    desc = _desc()
    for chunk in (100, 0, -64, 63, 65):
        rc, b = _ws_bytes(desc, chunk, 0)
        assert rc == -1 and b == -7, chunk                    # RNB_E_INVALID, nothing written
        assert b"multiple of 64" in lib.rnb_last_error_string()
    rc, _ = _ws_bytes(desc, 64, 4)
    assert rc == -1 and b"flag" in lib.rnb_last_error_string()
    assert lib.rnb_mesh_vertex_workspace_bytes(C.byref(desc), 64, 0, None) == -4   # RNB_E_NULL


def test_argument_checks_come_before_any_launch():
    """Every refusal below returns before the workspace or a stream is touched (ws is NULL throughout: a call that got as
    far as its workspace would answer RNB_E_NULL, one that launched would need a device)."""
    lib = R.native.load()
    desc = _desc()
    packed = C.c_void_p(256)       # never dereferenced on the host
    out = C.c_void_p(512)

    def call(chunk=64, **kw):
        a = R.native.MeshVertexArgs()
        a.points, a.V, a.sdf_out = 1024, 10, out
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.rnb_mesh_vertex_attrs(C.byref(desc), packed, C.byref(a), chunk, None, 0, None)

    assert call(chunk=100) == -1
    assert call(refine=-1) == -1
    assert call(refine=1, max_step=0.0) == -1 and b"max_step" in lib.rnb_last_error_string()
    assert call(refine=1, max_step=-1.0) == -1
    assert call(albedo_out=out) == -1 and b"RNB_MESH_ALBEDO" in lib.rnb_last_error_string()
    assert call(rgb_out=out) == -1
    assert call(flags=8) == -1
    assert call(V=-1) == -1
    assert call(sdf_out=None) == -1 and b"no output" in lib.rnb_last_error_string()
    assert call(grid_vertices=2048, resolution=1) == -1
    assert call(V=0) == 0                                      # nothing to do, nothing launched
    assert call(points=None) == -4                             # neither grid_vertices nor points
    assert call() == -4 and b"workspace" in lib.rnb_last_error_string()   # valid arguments reach the workspace check
    assert lib.rnb_mesh_vertex_attrs(C.byref(desc), packed, None, 64, None, 0, None) == -4


def test_renderer_argument_checks():
    mc, p, _ = U.model("tiny")
    sdf, dev, col, ren = R.build_from_named_params(mc, p, torch.device("cpu"))
    pts = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="either points or grid_vertices"):
        ren.vertex_attributes()
    with pytest.raises(ValueError, match="either points or grid_vertices"):
        ren.vertex_attributes(pts, grid_vertices=pts.double())
    with pytest.raises(ValueError, match="max_step"):
        ren.vertex_attributes(pts, refine=1)
    with pytest.raises(ValueError, match="bounds"):
        ren.vertex_attributes(grid_vertices=pts.double())
    with pytest.raises(ValueError, match="refine"):
        ren.vertex_attributes(pts, refine=-1)
    # a renderer without the albedo network: geometry only
    geo = R.NeuSRenderer(None, sdf, dev, None, n_samples=16, n_importance=16, n_outside=0, up_sample_steps=4, perturb=0.0)
    with pytest.raises(ValueError, match="albedo"):
        geo.vertex_attributes(pts, albedo=True)
    # there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        ren.vertex_attributes(pts)
