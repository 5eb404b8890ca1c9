"""The table of tests/adjoint_matrix.py on the CPU oracle alone (no GPU, no library): every condition the device test of
tests/test_gpu_adjoint_matrix.py relies on is a property of its inputs, checked here before any device code runs.  Per
row: the declared zero leaves are exactly the leaves whose fp64 gradient is None or zero, every other leaf has an fp64
gradient that does not vanish and that the fp32 oracle resolves to GRAD_CAP / K_GRAD; per shape: the weight_max selection
keeps at least half of the rays and the fp32 oracle's arg-max is the fp64 one on them."""
import pytest
import torch

from oracle import rnb_oracle as O
from tests import adjoint_matrix as M
from tests import parity as P


def test_the_table_is_what_it_says():
    names = {r.name for r in M.ROWS}
    for api in ("render", "render_rnb", "render_rnb_warmup"):
        for adj in M.ADJOINTS:
            assert f"w32-{api}-{adj}" in names
    assert "w32-render_rnb_no_albedo-color_fine" in names
    for adj in M.ADJOINTS + ("all",):
        assert f"default_64x64-render_rnb-{adj}" in names
    for adj in ("color_fine", "s_val", "weight_max"):
        assert f"default_64x64-render-{adj}" in names
    assert len(M.ROWS) == 3 * 8 + 1 + 9 + 3
    assert [r.api for r in M.ROWS if r.api == "render_rnb_no_albedo"] == ["render_rnb_no_albedo"]
    assert M.S == 80 and M.S > 64 and M.S % 64 == 16, "one carry and a ragged 16-lane chunk"
    assert M.COS_ANNEAL == 0.5 and M.BACKGROUND == (0.2, 0.5, 0.8)
    assert M.RAYS == {"w32": (16, 1), "default_64x64": (64, 2)}
    for r in M.ROWS:
        assert (r.api, r.adjoint) in M.ZERO_LEAVES
    for shape in M.RAYS:
        mc, p = M.model(shape)
        assert mc.render == O.RenderConf(n_samples=64, n_importance=16, up_sample_steps=1)
        assert set(p) == M.SDF_LEAVES | M.ALBEDO_LEAVES | {M.VARIANCE} and len(p) == 37
        assert set(O.param_order(mc)) == set(p)
    # lights: per ray for render_rnb, shared for the warm-up
    assert tuple(M.batch("w32", "render_rnb")["lights_dir"].shape) == (3, 16, 1, 3)
    assert tuple(M.batch("w32", "render_rnb_warmup")["lights_dir"].shape) == (3, 1, 1, 3)
    assert torch.equal(M.batch("w32", "render_rnb")["rays_d"], M.batch("w32", "render_rnb_warmup")["rays_d"])


@pytest.mark.parametrize("shape", list(M.RAYS))
def test_depths_and_surface(shape):
    z = M.depths(shape)
    assert z.dtype == torch.float32 and tuple(z.shape) == (M.RAYS[shape][0], 80)
    assert bool((z[:, 1:] >= z[:, :-1]).all()) and bool(torch.isfinite(z).all())
    out = M.oracle_outputs(shape, "render_rnb", torch.float64)
    assert torch.equal(out["z_vals"], z.double()), "the oracle must render at the depths it was given"
    assert float(out["weight_sum"].mean()) > 0.3 and float(out["weights"].max()) > 1e-2, "degenerate scene"
    if shape == "default_64x64":
        assert abs(float(out["weight_sum"].mean()) - 0.55) < 0.01


@pytest.mark.parametrize("shape", list(M.RAYS))
def test_weight_max_selection(shape):
    kept, arg64, margin = M.weight_max_selection(shape)
    B = M.RAYS[shape][0]
    w32 = M.oracle_outputs(shape, "render_rnb", torch.float32)["weights"]
    print(f"ADJ weight_max {shape}: {int(kept.sum())} of {B} rays kept (margin {margin:.3e})")
    assert kept.shape == (B,) and 2 * int(kept.sum()) >= B, f"{shape}: only {int(kept.sum())} of {B} rays kept"
    assert torch.equal(w32.argmax(dim=-1)[kept], arg64[kept]), "the fp32 oracle's arg-max differs from fp64 on a kept ray"
    # the selection is a property of the weights, which no light and no background enters
    for api in ("render", "render_rnb_warmup"):
        assert torch.equal(M.oracle_outputs(shape, api, torch.float64)["weights"],
                           M.oracle_outputs(shape, "render_rnb", torch.float64)["weights"])
    cot = M.cotangents(shape, "render_rnb")["weight_max"]
    assert torch.equal(cot[:, 0] != 0, kept)


def test_all_is_the_sum_of_the_single_rows():
    """one generator over all eight outputs whatever the adjoint: the cotangent of an output is the same in every row"""
    shape, api = "w32", "render_rnb"
    g_all = M.oracle_grads(M.AdjRow(shape, api, "all"), torch.float64)
    singles = [M.oracle_grads(M.AdjRow(shape, api, a), torch.float64) for a in M.ADJOINTS]
    for k, g in g_all.items():
        s = sum(x[k] for x in singles if x[k] is not None)
        assert P.rel_l2(s, g) < 1e-12, k
    cot = M.cotangents(shape, api)
    for k, c in cot.items():
        assert c.dtype == torch.float64 and (k == "weight_max" or abs(float(c.norm()) - 1.0) < 0.5)


@pytest.mark.parametrize("row", M.ROWS, ids=[r.name for r in M.ROWS])
def test_row_on_the_oracle(row):
    g64 = M.oracle_grads(row, torch.float64)
    g32 = M.oracle_grads(row, torch.float32)
    zero = {k for k, g in g64.items() if M.is_zero(g)}
    assert zero == set(M.zero_leaves(row)), \
        f"{row.name}: declared zero but live: {sorted(set(M.zero_leaves(row)) - zero)}; live but zero: {sorted(zero - set(M.zero_leaves(row)))}"
    worst = ("", 0.0)
    for k, g in g64.items():
        if k in zero:
            assert M.is_zero(g32[k]), f"{row.name}: {k} is zero in fp64 and not in fp32"
            continue
        assert bool(torch.isfinite(g).all())
        assert float(g.norm()) > 1e-9, f"{row.name}: {k}: the fp64 gradient vanishes ({float(g.norm()):.2e}): not a parity target"
        rel32 = P.rel_l2(g32[k], g)
        assert rel32 <= P.GRAD_CAP / P.K_GRAD, f"{row.name}: {k}: the fp32 oracle itself is {rel32:.2e} from fp64"
        if rel32 > worst[1]:
            worst = (k, rel32)
    print(f"ADJ {row.name}: {len(zero)} zero leaves of {len(g64)}; worst fp32-vs-fp64 rel-L2 {worst[1]:.2e} ({worst[0]})")


@pytest.mark.parametrize("variance,inside", M.CLIP_VARIANCES)
def test_variance_clip_rows_on_the_oracle(variance, inside):
    """exp(10 variance) lies where the row says, s_val is the clip value outside, d loss / d variance is exactly zero
    outside and live inside, and every other leaf is a parity target at these four states"""
    raw = float(torch.exp(torch.tensor(variance, dtype=torch.float64) * 10.0))
    assert (1e-6 < raw < 1e6) == inside
    if inside:
        assert min(abs(raw / 1e6 - 1.0), abs(raw / 1e-6 - 1.0)) < 1e-3, "just inside the clip"
    o64, g64 = M.clip_oracle(variance, torch.float64)
    o32, g32 = M.clip_oracle(variance, torch.float32)
    if not inside:
        want = 1e-6 if variance > 0 else 1e6
        torch.testing.assert_close(o64["s_val"], torch.full_like(o64["s_val"], want), rtol=1e-12, atol=0.0)
        assert M.is_zero(g64[M.VARIANCE]) and M.is_zero(g32[M.VARIANCE])
    worst = ("", 0.0)
    for k, g in g64.items():
        if k == M.VARIANCE and not inside:
            continue
        assert float(g.norm()) > 1e-9, f"variance {variance}: {k}: the fp64 gradient vanishes"
        rel32 = P.rel_l2(g32[k], g)
        assert rel32 <= P.GRAD_CAP / P.K_GRAD, f"variance {variance}: {k}: the fp32 oracle itself is {rel32:.2e} from fp64"
        if rel32 > worst[1]:
            worst = (k, rel32)
    print(f"ADJ clip variance {variance:+.4f}: raw inv_s {raw:.4e}, worst fp32-vs-fp64 rel-L2 {worst[1]:.2e} ({worst[0]})")
