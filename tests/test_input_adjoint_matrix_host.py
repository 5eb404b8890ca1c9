"""The table of tests/input_adjoint_matrix.py on the CPU oracle alone (no GPU, no library): every condition the device test
of tests/test_gpu_input_adjoint_matrix.py relies on is a property of its inputs, checked here before any device code runs.
Per row and input: a declared zero is the oracle's zero in fp64 and in fp32 (autograd finds no path, or the gradient is
exactly 0), every other one has an fp64 gradient that does not vanish and that the fp32 oracle resolves to
GRAD_CAP / K_GRAD — a condition: a host whose fp32 arithmetic refuses one fails here, nothing is skipped.  Under weight_max
the rows of the rays the selection drops are the oracle's zero rows and the kept rows are the parity target."""
import pytest
import torch

from tests import adjoint_matrix as M
from tests import input_adjoint_matrix as IM
from tests import parity as P


def test_the_table_is_what_it_says():
    names = [r.name for r in IM.INPUT_ROWS]
    assert names[:len(M.ROWS)] == [r.name for r in M.ROWS], "the parameter table's rows come first, unchanged"
    extra = set(names[len(M.ROWS):])
    want = ({f"default_64x64-render_rnb_no_albedo-{a}" for a in ("color_fine", "weights", "gradients", "gradient_error", "all")}
            | {f"default_64x64-render_rnb_warmup-{a}" for a in ("color_fine", "gradients", "all")}
            | {"default_64x64-render-all"}
            | {f"w32-render_rnb_no_albedo-{a}" for a in ("gradients", "weight_sum", "all")})
    assert extra == want and len(IM.INPUT_ROWS) == len(M.ROWS) + 12
    assert IM.INPUTS["render"] == ("rays_o", "rays_d", "z_vals", "background_rgb")
    for api in ("render_rnb", "render_rnb_warmup", "render_rnb_no_albedo"):
        assert IM.INPUTS[api] == ("rays_o", "rays_d", "z_vals", "lights_dir")
    for r in IM.INPUT_ROWS:
        z = IM.zero_inputs(r)
        assert z <= set(IM.inputs(r))
        if r.adjoint == "s_val":
            assert z == set(IM.inputs(r))
        elif r.adjoint in ("color_fine", "all"):
            assert not z
        else:
            assert z == set(IM.inputs(r)) - set(IM.RAY_INPUTS) and len(z) == 1
        assert (IM.zero_rays(r) is not None) == (r.adjoint == "weight_max")
    # shapes of the leaves: per-ray lights for render_rnb and no_albedo, shared for the warm-up
    x = IM.input_values("default_64x64", "render_rnb_no_albedo")
    assert tuple(x["lights_dir"].shape) == (3, 64, 1, 3) and tuple(x["z_vals"].shape) == (64, 80)
    assert tuple(IM.input_values("default_64x64", "render_rnb_warmup")["lights_dir"].shape) == (3, 1, 1, 3)
    assert tuple(IM.input_values("w32", "render")["background_rgb"].shape) == (3,)


@pytest.mark.parametrize("shape,api", sorted({(r.shape, r.api) for r in IM.INPUT_ROWS}))
def test_graph_keeping_normal_leaves_the_outputs_alone(shape, api):
    """the oracle with the inputs as leaves and the graph-keeping normal renders what the parameter table's oracle renders"""
    for dt in (torch.float64, torch.float32):
        mine, theirs = IM.oracle_outputs(shape, api, dt), M.oracle_outputs(shape, api, dt)
        for k in M.ADJOINTS:
            if api == "render" and k == "color_fine" and dt == torch.float64:
                # the background here is the fp32 tensor the device is handed, there the same three numbers in fp64
                assert P.max_err(mine[k], theirs[k]) < 1e-7
                continue
            assert torch.equal(mine[k], theirs[k]), f"{shape} {api} {dt}: {k} differs"
    assert torch.equal(IM.oracle_outputs(shape, api, torch.float64)["z_vals"], M.depths(shape).double())


@pytest.mark.parametrize("shape", list(M.RAYS))
def test_weight_max_rows(shape):
    """the dropped rays are those of adjoint_matrix.weight_max_selection (tests/test_adjoint_matrix_host.py holds its
    counts); their rows of every ray input are exactly zero on the oracle, in both dtypes"""
    kept, _, _ = M.weight_max_selection(shape)
    B = M.RAYS[shape][0]
    for api in ("render", "render_rnb", "render_rnb_warmup"):
        row = IM.BY_NAME.get(f"{shape}-{api}-weight_max")
        if row is None:
            continue
        dropped = IM.zero_rays(row)
        assert torch.equal(dropped, ~kept) and 0 < int(dropped.sum()) and 2 * int(kept.sum()) >= B
        for dt in (torch.float64, torch.float32):
            g = IM.oracle_input_grads(row, dt)
            for k in IM.RAY_INPUTS:
                assert not bool((g[k][dropped] != 0).any()), f"{row.name} {dt}: {k} is live on a dropped ray"
                assert bool((g[k][kept] != 0).any(dim=-1).all()), f"{row.name} {dt}: {k} is dead on a kept ray"
    print(f"INADJ weight_max {shape}: {int(kept.sum())} of {B} rays kept, {B - int(kept.sum())} rows exactly zero")


@pytest.mark.parametrize("shared", [False, True], ids=["per_ray", "shared"])
def test_no_albedo_lights_of_both_shapes(shared):
    """default_64x64 / render_rnb_no_albedo / color_fine with per-ray [L,B,1,3] and shared [L,1,1,3] lights: lights_dir.grad
    has the lights' shape, does not vanish and is resolved by the fp32 oracle, and so are the ray inputs"""
    row = IM.BY_NAME["default_64x64-render_rnb_no_albedo-color_fine"]
    want = (3, 1, 1, 3) if shared else (3, 64, 1, 3)
    assert tuple(IM.input_values(row.shape, row.api, shared)["lights_dir"].shape) == want
    g64 = IM.oracle_input_grads(row, torch.float64, shared)
    g32 = IM.oracle_input_grads(row, torch.float32, shared)
    assert tuple(g64["lights_dir"].shape) == want
    for k, g in g64.items():
        assert float(g.norm()) > 1e-9, k
        rel32 = P.rel_l2(g32[k], g)
        assert rel32 <= P.GRAD_CAP / P.K_GRAD, f"{k}: the fp32 oracle itself is {rel32:.2e} from fp64"
    if not shared:
        assert torch.equal(g64["lights_dir"], IM.oracle_input_grads(row, torch.float64)["lights_dir"])


def test_all_is_the_sum_of_the_single_rows():
    shape, api = "default_64x64", "render_rnb"
    g_all = IM.oracle_input_grads(IM.BY_NAME[f"{shape}-{api}-all"], torch.float64)
    singles = [IM.oracle_input_grads(IM.BY_NAME[f"{shape}-{api}-{a}"], torch.float64) for a in M.ADJOINTS]
    for k, g in g_all.items():
        s = sum(x[k] for x in singles if x[k] is not None)
        assert P.rel_l2(s, g) < 1e-12, k


@pytest.mark.parametrize("row", IM.INPUT_ROWS, ids=[r.name for r in IM.INPUT_ROWS])
def test_row_on_the_oracle(row):
    g64 = IM.oracle_input_grads(row, torch.float64)
    g32 = IM.oracle_input_grads(row, torch.float32)
    assert tuple(g64) == IM.inputs(row)
    zero = {k for k, g in g64.items() if IM.is_zero(g)}
    declared = set(IM.zero_inputs(row))
    assert zero == declared, f"{row.name}: declared zero but live: {sorted(declared - zero)}; live but zero: {sorted(zero - declared)}"
    dropped = IM.zero_rays(row)
    notes = []
    for k, g in g64.items():
        if k in zero:
            assert IM.is_zero(g32[k]), f"{row.name}: {k} is zero in fp64 and not in fp32"
            continue
        a, r = g32[k], g
        assert a.shape == r.shape == IM.input_values(row.shape, row.api)[k].shape
        if dropped is not None:
            a, r = a[~dropped], r[~dropped]
        assert bool(torch.isfinite(r).all())
        assert float(r.norm()) > 1e-9, f"{row.name}: {k}: the fp64 gradient vanishes ({float(r.norm()):.2e}): not a parity target"
        rel32 = P.rel_l2(a, r)
        notes.append(f"{k} |g| {float(r.norm()):.2e} fp32-vs-fp64 {rel32:.2e}")
        assert rel32 <= P.GRAD_CAP / P.K_GRAD, f"{row.name}: {k}: the fp32 oracle itself is {rel32:.2e} from fp64"
    print(f"INADJ {row.name}: zero {sorted(zero)}; " + "; ".join(notes))
