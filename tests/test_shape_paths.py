"""The shape table of tests/shape_matrix.py against the library's own host-side layout queries (no GPU): every entry is
accepted, takes the path the table names (fused x2h or per-layer generic), is accepted or refused by RNB_VARIANT_BF16 as
the table says, and its test state (live_params) is non-degenerate.  This pins the table that tests/test_gpu_shapes.py
runs on the device: a shape cannot be tested as "fused" while the library sends it down the generic path."""
import ctypes as C

import pytest
import torch

import rnb_neus_fork_amd as R
from oracle import rnb_oracle as O
from oracle.bf16_emu import packed_layout
from tests.gpu_support import assert_has_surface
from tests.shape_matrix import SHAPES, desc_of, live_params, oracle_points, pe_columns, points, step_batch, zero_blocks


def _packed_floats(mc, **variant):
    lib = R.native.load()
    n = C.c_int64(-1)
    rc = lib.rnb_packed_floats(C.byref(desc_of(mc, **variant)), C.byref(n))
    return rc, n.value, lib.rnb_last_error_string().decode()


@pytest.mark.parametrize("shape", SHAPES, ids=[s.name for s in SHAPES])
def test_shape_takes_the_tabled_path(shape):
    mc = shape.mc
    L = packed_layout(mc)
    total = L["total"]
    rc, n_default, err = _packed_floats(mc)
    assert rc == 0, f"{shape.name}: rejected: {err}"
    rc, n_generic, err = _packed_floats(mc, generic=True)
    assert rc == 0, err
    assert n_generic == total, "RNB_VARIANT_GENERIC: the fp32 weights alone (oracle/bf16_emu.packed_layout)"
    # the default of a fused shape carries the x3 mirror (1.5 x), the x2h fp16 planes (1 x) and their scale table: the
    # arithmetic of test_packed_layout_size_and_workspace_queries, for this shape
    x2h_size = total + total // 2 * 3 + total + 256
    path = "x2h" if n_default == x2h_size else "generic" if n_default == total else f"unknown ({n_default} floats)"
    assert path == shape.path, f"{shape.name}: the library takes the {path} path, the table says {shape.path}"
    rc, n_bf16, err = _packed_floats(mc, bf16=True)
    if shape.bf16:
        assert rc == 0, f"{shape.name}: RNB_VARIANT_BF16 rejected: {err}"
        assert n_bf16 == total + total // 2, "RNB_VARIANT_BF16: fp32 weights + one bf16 mirror"
    else:
        assert rc == -1 and "RNB_VARIANT_BF16" in err, f"{shape.name}: RNB_VARIANT_BF16 must be refused (rc {rc})"
    # the rules of color_h2_supported (color_h2.hip) and sweep_mv_supported (sweep_mv.hip) on this layout
    Ep = (shape.pe + 31) // 32 * 32
    cc = mc.color
    color_h2 = (shape.fused and L["F"] == 256 and cc.n_layers == 2 and cc.d_hidden == 256 and Ep == 64
                and L["Cinp"] - L["F"] == 64 and 1 <= cc.d_out <= 4)
    assert color_h2 == shape.color_h2, shape.name
    mv = (shape.fused and Ep == 64 and 2 <= mc.sdf.n_layers <= 8 and all(e["N"] >= 192 for e in L["hid"])
          and (L["F"] == 0 or (L["feat"]["Np"] == 256 and L["F"] % 4 == 0)))
    assert mv == shape.mv, shape.name


@pytest.mark.parametrize("shape", SHAPES, ids=[s.name for s in SHAPES])
def test_shape_state_is_live_and_the_oracle_resolves_it(shape):
    """live_params: no zero block, PE columns live, variance in [0.3, 0.4]; the fp32 oracle within a few ulps of the fp64
    one on a few points (so the calibrated bounds of the GPU tests are not set by a degenerate yardstick); and the step
    batch renders a surface (tests/gpu_support.py assert_has_surface, on the oracle's own sampling)."""
    mc = shape.mc
    p = live_params(mc, shape.seed)
    assert zero_blocks(p, mc) == [], shape.name
    cols = pe_columns(p, mc)
    assert (len(cols) > 0) == (mc.sdf.multires > 0)
    assert len(cols) == (1 + len(mc.sdf.skip_in) if mc.sdf.multires > 0 else 0)
    assert 0.3 <= float(p["dev.variance"]) <= 0.4
    pts = points(17, seed=5)
    gen = torch.Generator().manual_seed(6)
    nrm = torch.randn(17, 3, generator=gen)
    feats = torch.randn(17, mc.color.d_feature, generator=gen) * 0.3
    r64 = oracle_points(p, mc, pts, nrm, feats, torch.float64)
    r32 = oracle_points(p, mc, pts, nrm, feats, torch.float32)
    for name, a, b in zip(("sdf+feature", "normal", "albedo"), r32, r64):
        assert a.shape == b.shape
        torch.testing.assert_close(a.double(), b, rtol=1e-5, atol=1e-5, msg=lambda m: f"{shape.name} {name}: {m}")
    if shape.render:
        b = step_batch()
        with torch.no_grad():
            out = O.render_rnb(p, mc, b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=1.0,
                               t_rand=b["t_rand"])
        assert_has_surface(out)
