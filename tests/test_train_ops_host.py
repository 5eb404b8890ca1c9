"""tests/train_ops_ref.py pinned on the host (no GPU): the references of the loss, Adam and weight-norm kernels against the
oracle and torch, and every condition tests/test_gpu_train_ops_edges.py and tests/test_gpu_weightnorm.py place on their
inputs, so that the device tests cannot pass on a degenerate yardstick."""
import numpy as np
import pytest
import torch

from oracle import rnb_oracle as O
from oracle.bf16_emu import packed_layout, weights_from_packed, weights_from_params
from tests import train_ops_ref as T
from tests.shape_matrix import BY_NAME, live_params


# ----------------------------------------------------------------------------------------------------------------- loss
def test_clip_bounds_are_the_fp32_numbers():
    assert np.float32(1.0) - np.float32(1e-3) == np.float32(0.999)
    assert T.CLIP_HI > 0.999 and T.CLIP_HI == float(np.float32(0.999))
    assert T.CLIP_LO == float(np.float32(1e-3)) and T.CLIP_LO != 1e-3
    # what torch's fp32 clip does with the reference's double constants: the same two numbers
    x = torch.tensor([0.0, 1.0]).clip(1e-3, 1.0 - 1e-3)
    assert float(x[0]) == T.CLIP_LO and float(x[1]) == T.CLIP_HI


def test_loss_shapes_cover_the_listed_values():
    assert {s[0] for s in T.LOSS_SHAPES} == {1, 63, 65, 1023, 1024, 1025, 4099}
    assert {s[1] for s in T.LOSS_SHAPES} == {1, 2, 5} and {s[2] for s in T.LOSS_SHAPES} == {1, 3, 4}
    assert (1025, 5, 4) in T.LOSS_SHAPES
    assert sum(T.LOSS_SHARDS) == 128


@pytest.mark.parametrize("shape", T.LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mask_w", [T.MASK_W, 0.0])
def test_loss_ref_fp32_is_the_oracle(shape, mask_w):
    """values and all three gradients, bit for bit: loss_ref in fp32 runs the oracle's own operations"""
    B, L, Cd = shape
    color, rgb, mask, ws, ge = T.loss_inputs(B, L, Cd, seed=B + L)
    got = T.loss_ref_run((color, rgb, mask, ws, ge), T.IGR_W, mask_w, torch.float32, upstream=1.7)
    leaves = [t.clone().requires_grad_(True) for t in (color, ws.reshape(-1, 1), ge)]
    ref, parts = O.rnb_loss({"color_fine": leaves[0], "weight_sum": leaves[1], "gradient_error": leaves[2]}, rgb,
                            mask.reshape(-1, 1), igr_weight=T.IGR_W, mask_weight=mask_w)
    (ref * 1.7).backward()
    assert torch.equal(got["loss"], ref.detach())
    for k in ("color_loss", "eikonal_loss", "mask_loss"):
        assert torch.equal(got[k], parts[k].detach()), k
    assert torch.equal(got["d_color"], leaves[0].grad)
    assert torch.equal(got["d_ws"], leaves[1].grad.reshape(-1))
    assert torch.equal(got["d_ge"], leaves[2].grad)


def test_loss_inputs_hold_every_edge():
    color, rgb, mask, ws, ge = T.loss_inputs(63, 2, 3, seed=65)
    edges = T.weight_sum_edges()
    lo, hi = np.float32(T.CLIP_LO), np.float32(T.CLIP_HI)
    assert len(edges) == 12 and float(edges[2]) > 0.0
    assert float(edges[3]) < lo == float(edges[4]) < float(edges[5])
    assert float(edges[7]) < hi == float(edges[8]) < float(edges[9])
    assert torch.equal(ws[:12], edges) and torch.equal(ws[12:24], edges)
    assert bool((mask[:12] == 1).all()) and bool((mask[12:24] == 0).all())
    assert set(mask.tolist()) == set(torch.tensor(T.MASK_VALUES).tolist()) and len(set(T.MASK_VALUES)) == 6
    assert T.MASK_VALUES[3] > 0.5 and np.float32(T.MASK_VALUES[3]) == np.nextafter(np.float32(0.5), np.float32(1))
    e = color - rgb
    assert bool((e[:, 33] == 0).all())
    assert bool((e[:, 34] == 0).all()) and bool(torch.signbit(e[:, 34]).all())       # -0.0 differences
    assert float(e[0, 35, 0]) == 0.0 and float(mask[35]) == 1.0
    r64 = T.loss_ref_run((color, rgb, mask, ws, ge), T.IGR_W, T.MASK_W, torch.float64)
    d = r64["d_ws"]
    # the sub-gradient of clip is inclusive: zero strictly outside, the BCE derivative on the bounds
    outside = [0, 1, 2, 3, 9, 10, 11]
    inside = [4, 5, 6, 7, 8]
    for base in (0, 12):
        assert bool((d[[base + i for i in outside]] == 0).all())
        assert bool((d[[base + i for i in inside]] != 0).all())
    assert bool((r64["d_color"][:, 33] == 0).all()) and bool((r64["d_color"][:, 34] == 0).all())
    assert float(r64["d_color"][0, 35, 0]) == 0.0


def test_loss_mask_extremes():
    inp = T.loss_inputs(65, 2, 3, seed=1, mask_mode="zeros")
    r = T.loss_ref_run(inp, T.IGR_W, T.MASK_W, torch.float64)
    assert float(r["color_loss"]) == 0.0 and bool((r["d_color"] == 0).all())
    inp = T.loss_inputs(65, 2, 3, seed=1, mask_mode="ones")
    r1 = T.loss_ref_run(inp, T.IGR_W, T.MASK_W, torch.float64)
    assert float(r1["color_loss"]) > 0.0
    r0 = T.loss_ref_run(T.loss_inputs(65, 2, 3, seed=1), T.IGR_W, 0.0, torch.float64)   # mask_weight 0: mask ignored
    assert float(r0["color_loss"]) == float(r1["color_loss"]) and bool((r0["d_ws"] == 0).all())


def test_loss_non_finite_cases_poison_what_they_should():
    B, L, Cd = 65, 2, 3
    r = T.loss_ref_run(T.loss_inputs(B, L, Cd, seed=2, special="nan_ws"), T.IGR_W, T.MASK_W, torch.float64)
    assert torch.isnan(r["mask_loss"]) and torch.isnan(r["loss"]) and torch.isfinite(r["color_loss"])
    assert bool(torch.isfinite(r["d_color"]).all()) and bool(torch.isfinite(r["d_ws"][:B - 1]).all())
    r = T.loss_ref_run(T.loss_inputs(B, L, Cd, seed=2, special="inf_color"), T.IGR_W, T.MASK_W, torch.float64)
    assert torch.isinf(r["color_loss"]) and torch.isinf(r["loss"]) and torch.isfinite(r["mask_loss"])
    assert bool(torch.isfinite(r["d_color"]).all()) and bool(torch.isfinite(r["d_ws"]).all())


@pytest.mark.parametrize("mask_w", [T.MASK_W, 0.0])
def test_loss_shard_shares_add_up(mask_w):
    inp = T.loss_inputs(128, 2, 3, seed=128)
    color, rgb, mask, ws, ge = inp
    whole = T.loss_ref_run(inp, T.IGR_W, mask_w, torch.float64)
    count = float((mask > 0.5).sum()) if mask_w > 0 else 128.0
    assert 0 < count <= 128
    tot = {k: 0.0 for k in ("loss", "color_loss", "eikonal_loss", "mask_loss")}
    dc, dw, b0 = [], [], 0
    for n in T.LOSS_SHARDS:
        sl = slice(b0, b0 + n)
        r = T.loss_ref_run((color[:, sl], rgb[:, sl], mask[sl], ws[sl], ge), T.IGR_W, mask_w, torch.float64,
                           batch_global=(count, 128.0), eik_share=1.0 / 3.0)
        for k in tot:
            tot[k] += float(r[k])
        dc.append(r["d_color"])
        dw.append(r["d_ws"])
        b0 += n
    for k in tot:
        assert tot[k] == pytest.approx(float(whole[k]), rel=1e-13), k
    torch.testing.assert_close(torch.cat(dc, 1), whole["d_color"], rtol=1e-13, atol=0)
    torch.testing.assert_close(torch.cat(dw), whole["d_ws"], rtol=1e-13, atol=0)


# ----------------------------------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("setting", list(T.ADAM_SETTINGS))
def test_adam_ref_is_torch_adam_in_fp64(setting):
    betas, eps, wd, _ = T.ADAM_SETTINGS[setting]
    steps = 60
    seq = T.adam_grad_sequence(steps).reshape(steps, -1)
    lrs = [T.adam_lr(it, steps) for it in range(steps)]
    p0 = T.adam_params0().reshape(-1)
    p, m, v = T.adam_ref(p0, seq, lrs, betas, eps, wd, torch.float64)
    tp, tm, tv, _ = T.torch_adam_run(p0[None], seq[:, None], lrs, betas, eps, wd, torch.float64)
    torch.testing.assert_close(p, tp[0], rtol=1e-12, atol=1e-15)
    # (torch forms exp_avg as a lerp: an entry that cancels differs in its last digits, so the moments go by norm)
    assert T.rel_l2(m, tm[0]) < 1e-14 and T.rel_l2(v, tv[0]) < 1e-14


def test_adam_gradient_sequence_conditions():
    seq = T.adam_grad_sequence(2000)
    assert seq.dtype == torch.float32 and tuple(seq.shape) == (2000, 4, T.ADAM_NUMEL)
    assert min(T.ADAM_SCALES) >= 1e-12
    assert bool((seq[:, :, :T.ADAM_ZERO_HEAD] == 0).all())
    live = seq[:, :, T.ADAM_ZERO_HEAD:]
    tiny = float(np.finfo(np.float32).tiny)
    sq = live * live                                   # fp32, as the kernel squares it
    assert bool((sq >= tiny).all()), "g^2 must stay a normal fp32 number in every group"
    assert bool(torch.isfinite(sq).all())
    for k, s in enumerate(T.ADAM_SCALES):
        assert 0.5 * s < float(live[:, k].double().std()) < 2.0 * s
    assert torch.equal(T.adam_grad_sequence(500), seq[:500])


@pytest.mark.parametrize("setting", list(T.ADAM_SETTINGS))
def test_adam_long_run_yardstick_is_not_zero(setting):
    """the fp32 torch run differs from fp64 in every tensor's parameters and moments (so K_OUT times that distance is a
    bound, not zero), and the derived moment floor is what the issue of the kernel's `1.f - beta` gives"""
    betas, eps, wd, steps = T.ADAM_SETTINGS[setting]
    (p64, m64, v64), (p32, m32, v32) = T.adam_long_refs(setting)
    assert steps == (2000 if setting in ("default", "decay") else 500)
    for k in range(len(T.ADAM_SCALES)):
        assert float((p32[k].double() - p64[k]).abs().max()) > 0.0, k
        assert T.rel_l2(m32[k], m64[k]) > 0.0 and T.rel_l2(v32[k], v64[k]) > 0.0, k
        assert float(m64[k].norm()) > 0 and float(v64[k].norm()) > 0
        if wd == 0.0:     # a zero gradient never moves a parameter
            assert torch.equal(p64[k, :T.ADAM_ZERO_HEAD], T.adam_params0()[k, :T.ADAM_ZERO_HEAD].double())
        else:
            assert not torch.equal(p64[k, :T.ADAM_ZERO_HEAD], T.adam_params0()[k, :T.ADAM_ZERO_HEAD].double())
    assert T.adam_moment_floor(0.999) == pytest.approx(2.4e-4, rel=0.02)
    assert T.adam_moment_floor(0.9) == pytest.approx(2.4e-6, rel=0.02)
    # 1.f - beta2 in fp32 against the double 1 - beta2: the 1.3e-5 relative the floor is derived from
    off = abs(float(np.float32(1) - np.float32(0.999)) - (1 - 0.999)) / (1 - 0.999)
    assert 1e-5 < off < 2.0 ** -24 / (1 - 0.999)


# ---------------------------------------------------------------------------------------------------------- weight norm
WN = [BY_NAME[n] for n in T.WN_SHAPES]


def _scatter(effs, total, dtype=torch.float32):
    P = torch.zeros(total, dtype=dtype)
    for e in effs:
        P[e.w_slots] = e.W.detach().to(dtype)
        P[e.b_slots] = e.b.detach().reshape(-1).to(dtype)
    return P


@pytest.mark.parametrize("shape", WN, ids=lambda s: s.name)
def test_wn_effective_is_weights_from_params_and_its_slots_are_the_layout(shape):
    mc = shape.mc
    p = T.wn_params(shape, zero_row=False)
    effs = T.wn_effective(p, mc, torch.float64)
    ref = weights_from_params(p, mc, torch.float64)
    by = {e.name: e for e in effs}
    for l, w in enumerate(ref["W"]):
        assert torch.equal(by[f"sdf.lin{l}"].W, w) and torch.equal(by[f"sdf.lin{l}"].b, ref["b"][l])
    assert torch.equal(by["sdf.head"].W[0], ref["wsdf"]) and torch.equal(by["sdf.head"].b, ref["bsdf"])
    assert torch.equal(by["sdf.feat"].W, ref["Wf"]) and torch.equal(by["sdf.feat"].b, ref["bf"])
    for l, w in enumerate(ref["Wc"]):
        assert torch.equal(by[f"color.lin{l}"].W, w) and torch.equal(by[f"color.lin{l}"].b, ref["bc"][l])
    # the slots: distinct, inside their blocks, and read back by weights_from_packed (which undoes the albedo layer 0
    # column permutation and splits the output layer into the sdf row and the feature head)
    L = packed_layout(mc)
    slots = torch.cat([t.reshape(-1) for e in effs for t in (e.w_slots, e.b_slots)]
                      + [e.wT_slots.reshape(-1) for e in effs if e.wT_slots is not None])
    assert len(torch.unique(slots)) == len(slots) and int(slots.min()) >= 0 and int(slots.max()) < L["total"]
    assert not bool(T.allowed_unwritten(mc)[slots].any())
    back = weights_from_packed(_scatter(effs, L["total"], torch.float64).float(), mc)
    for k in ("W", "b", "Wc", "bc"):
        for a, b in zip(back[k], ref[k]):
            assert torch.equal(a, b.float()), k
    for k in ("wsdf", "bsdf", "Wf", "bf"):
        assert torch.equal(back[k], ref[k].float()), k
    # the blocks tile [0, end) without gaps: real slots + padding + transposes + bsdf[1:32] + tail = total
    regs, end = T.packed_regions(mc)
    covered = sum(n * k + nb + (n * k if wT is not None else 0) for _, _, n, k, _, nb, wT in regs)
    assert covered + 31 == end and (end + 31) // 32 * 32 == L["total"]
    assert int(T.allowed_unwritten(mc).sum()) == 31 + L["total"] - end


@pytest.mark.parametrize("shape", WN, ids=lambda s: s.name)
def test_wn_row_edits_and_the_misrounding_cap(shape):
    mc = shape.mc
    p = T.wn_params(shape, zero_row=True)
    layers = T.edited_layers(mc)
    assert len(layers) == (0 if shape.name == "no_weight_norm" else 2)
    effs = {e.name: e for e in T.wn_effective(p, mc, torch.float64)}
    plain = {e.name: e for e in T.wn_effective(live_params(mc, shape.seed), mc, torch.float64)}
    for pre in layers:
        g, v, W = p[pre + ".weight_g"], p[pre + ".weight_v"], effs[pre].W
        assert float(g[T.ROW_G_ZERO]) == 0.0 and float(g[T.ROW_G_NEG]) < 0.0
        assert bool((W[T.ROW_G_ZERO] == 0).all())
        assert 0 < float(v[T.ROW_V_TINY].abs().max()) < 1e-10 and float(v[T.ROW_V_HUGE].abs().max()) > 1e9
        assert float(W[T.ROW_V_TINY].abs().max()) > 1e-3 and float(W[T.ROW_V_HUGE].abs().max()) > 1e-3
        # scaling a v row leaves its W alone but for the fp32 rounding of the scaled v: each element moves by at most 2^-24
        # relative, and so does the row norm
        for row in (T.ROW_V_TINY, T.ROW_V_HUGE):
            assert float((W[row] - plain[pre].W[row]).abs().max()) <= 4 * 2.0 ** -24 * float(W[row].abs().max())
        nan_rows = torch.isnan(W).any(dim=1)
        assert bool(torch.isnan(W[T.ROW_V_ZERO]).all()) and int(nan_rows.sum()) == 1
    # the cap on entries that differ from float32(fp64 product): a second fp64 summation order of ||v||^2 (256 strided
    # partial sums, as a 256-thread block forms them) followed by one rounding must stay inside it
    p = T.wn_params(shape, zero_row=False)
    differ = total = 0
    for e in T.wn_effective(p, mc, torch.float64):
        if e.prefix + ".weight_g" not in p:
            continue
        g, v = p[e.prefix + ".weight_g"].double()[e.rows], p[e.prefix + ".weight_v"].double()[e.rows]
        K = v.shape[1]
        pad = (-K) % 256
        sq = torch.cat([v * v, torch.zeros(v.shape[0], pad, dtype=torch.float64)], 1).reshape(v.shape[0], -1, 256)
        ss = sq.sum(1).flip(-1).sum(-1, keepdim=True)
        scale = float(e.W.abs().max() / (v * (g / v.norm(dim=1, keepdim=True))).abs().max())     # 1 or 1 / sqrt(2)
        W2 = (v * (scale * (g / ss.sqrt()))).float()
        d = T.ulp_distance(W2, e.W.float())
        assert int(d.max()) <= 1
        differ += int((d != 0).sum())
        total += d.numel()
    print(f"{shape.name}: {differ} of {total} entries differ between two fp64 summation orders")
    assert differ <= T.WN_MISROUND_CAP * max(total, 1)


@pytest.mark.parametrize("shape", WN, ids=lambda s: s.name)
def test_wn_objective_gradients_have_a_yardstick(shape):
    """section 3b's reference: finite in fp64 and fp32, every real slot weighted, and the scaled rows' dv scale inversely"""
    mc = shape.mc
    L = packed_layout(mc)
    p = T.wn_params(shape, zero_row=False)
    c = torch.randn(L["total"], generator=torch.Generator().manual_seed(3))
    grads = {}
    for dt in (torch.float64, torch.float32):
        q = {k: v.clone().to(dt).requires_grad_(True) for k, v in p.items() if k != "dev.variance"}
        effs = T.wn_effective(q, mc, dt)
        for e in effs:
            assert bool((c[e.w_slots] != 0).all()) and bool((c[e.b_slots] != 0).all())
        T.wn_objective(effs, c, dt).backward()
        grads[dt] = {k: v.grad for k, v in q.items()}
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads[dt].values())
    for pre in T.edited_layers(mc):
        dv = grads[torch.float64][pre + ".weight_v"]
        typical = float(dv[10:].abs().max())
        assert float(dv[T.ROW_V_TINY].abs().max()) > 1e9 * typical * 1e-3
        assert 0 < float(dv[T.ROW_V_HUGE].abs().max()) < 1e-9 * typical * 1e3
        assert bool((dv[T.ROW_G_ZERO] == 0).all())
        assert float(grads[torch.float64][pre + ".weight_g"][T.ROW_G_ZERO].abs()) > 0
