"""Host-side checks of the sparse SDF grid: the binding against include/rnbneus.h, the brick geometry helper, and the argument
validation of `NeuSRenderer.extract_fields_sparse` that needs no device."""
import ctypes as C
import os
import re

import pytest
import torch

import rnb_neus_fork_amd as R
from oracle import rnb_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPARSE_CALLS = ["rnb_sdf_grid_sparse_workspace_bytes", "rnb_sdf_grid_sparse_seed", "rnb_sdf_grid_sparse_round",
                "rnb_sdf_grid_sparse_finish"]


def _header():
    return open(os.path.join(ROOT, "include", "rnbneus.h")).read()


def test_binding_matches_the_header():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"typedef struct rnb_sparse_grid_desc \{(.*?)\} rnb_sparse_grid_desc;", text, flags=re.S)
    assert m, "rnb_sparse_grid_desc is not declared"
    fields = [(t, n) for t, n in re.findall(r"(int32_t|float)\s+(\w+);", m.group(1))]
    assert fields == [("int32_t", "brick"), ("float", "threshold"), ("float", "margin")]
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(R.native.SparseGridDesc._fields_)
    assert C.sizeof(R.native.SparseGridDesc) == 12
    for name in SPARSE_CALLS:
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\);", text, flags=re.S)
        assert decl, f"{name} is not declared"
        assert name in R.native.EXPORTED_SYMBOLS
        restype, argtypes = R.native._SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == decl.group(1).count(",") + 1, name
    lib = R.native.load()
    assert lib.rnb_abi_version() == 5 and all(hasattr(lib, n) for n in SPARSE_CALLS)


@pytest.mark.parametrize("res,brick,nb,lattice,rows", [
    (70, 8, 9, [0, 8, 16, 24, 32, 40, 48, 56, 64, 69], 768),          # short last brick: 5 cells
    (97, 8, 12, list(range(0, 97, 8)), 768),                          # bricks tile the grid exactly
    (257, 16, 16, list(range(0, 257, 16)), 4928),
    (2, 4, 1, [0, 1], 128),                                           # one cell, one (short) brick
])
def test_brick_geometry(res, brick, nb, lattice, rows):
    g = R.native.brick_geometry(res, brick)
    assert g == {"nb": nb, "lattice": lattice, "samples": brick + 1, "rows": rows, "bricks_total": nb ** 3}
    # every cell lies in exactly one brick, every brick has at least one cell, the lattice ends on the last sample
    assert (nb - 1) * brick < res - 1 <= nb * brick and g["lattice"][-1] == res - 1 and len(g["lattice"]) == nb + 1
    assert g["rows"] % 64 == 0 and 0 <= g["rows"] - (brick + 1) ** 3 < 64


def test_brick_geometry_refuses_what_the_library_refuses():
    for res, brick in ((1, 8), (0, 8), (70, 5), (70, 0), (70, 64), (70, -8)):
        with pytest.raises(ValueError):
            R.native.brick_geometry(res, brick)


def test_extract_fields_sparse_validates_before_touching_a_device():
    mc = O.ModelConf(sdf=O.SDFConf(d_out=65, d_hidden=64), color=O.ColorConf(d_feature=64, d_hidden=64))
    torch.manual_seed(0)
    ren = R.build_from_named_params(mc, O.init_params(mc), torch.device("cpu"))[3]
    lo, hi = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="brick"):
        ren.extract_fields_sparse(lo, hi, 64, brick=5)
    with pytest.raises(ValueError, match="no cells"):
        ren.extract_fields_sparse(lo, hi, 1)
    for margin in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="margin"):
            ren.extract_fields_sparse(lo, hi, 64, margin=margin)
    with pytest.raises(ValueError, match="threshold"):
        ren.extract_fields_sparse(lo, hi, 64, threshold=float("nan"))
    with pytest.raises(ValueError, match="32-bit"):
        ren.extract_fields_sparse(lo, hi, 6000, brick=4)
    ren.set_data_parallel(group=object())
    with pytest.raises(ValueError, match="data-parallel"):
        ren.extract_fields_sparse(lo, hi, 64)
    with pytest.raises(ValueError, match="data-parallel"):
        ren.extract_geometry(lo, hi, 64, backend="native", sparse=True)
    ren.set_data_parallel(enabled=False)
    with pytest.raises(RuntimeError, match="GPU tensors only"):   # a CPU model: there is no CPU path
        ren.extract_fields_sparse(lo, hi, 64)
    assert R.renderer.DEFAULT_SPARSE_BRICK in R.native.SPARSE_BRICKS and ren.last_sparse_grid is None
