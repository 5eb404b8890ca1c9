"""rnb_loss_kernel and adam_kernel (csrc/train.hip) called directly, against the fp64 references of tests/train_ops_ref.py,
at the shapes and values where they can break.  tests/test_train_ops_host.py pins the references and the inputs.

Rule for a value: the output rule of tests/parity.py (ref32 is the same reference in fp32 on the CPU),
for the loss, each of its three parts, and each gradient tensor by max-abs.  Every case prints its errors as fractions of
their bounds in lines starting with TRAINOPS (the lines profiles/train_ops_edges.txt is for)."""
import pytest
import torch

from tests import parity as P
from tests import train_ops_ref as T
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device

pytestmark = pytest.mark.gpu

PARTS = ("color_loss", "eikonal_loss", "mask_loss")
RNB_E_INVALID = -1


def _rule(tag, name, dev, r64, r32):
    """the value rule on one scalar or (by max-abs) one tensor; returns error / bound"""
    r64 = r64.double()
    e_dev, e_ref, bound = P.value_errors(dev, r64, r32)
    print(f"TRAINOPS {tag} {name}: |dev - fp64| {e_dev:.3e}  fp32 ref {e_ref:.3e}  bound {bound:.3e}  ratio {e_dev / bound:.3f}")
    return P.check_value(f"{tag} {name}", dev, r64, r32)


# ----------------------------------------------------------------------------------------------------------------- loss
def _loss_direct(R, inp, igr_w, mask_w, batch_global=None, eik_share=1.0):
    """rnb_loss_rnb (or rnb_loss_rnb_shard with batch_global) on fp32 inputs; outputs pre-filled with NaN"""
    lib = R.native.load()
    d = device()
    color, rgb, mask, ws, ge = [t.to(torch.float32).contiguous().to(d) for t in inp]
    L, B, Cd = color.shape
    ge = ge.reshape(1)
    nan = float("nan")
    loss = torch.full((1,), nan, device=d)
    parts = torch.full((3,), nan, device=d)
    d_color = torch.full((L, B, Cd), nan, device=d)
    d_ws = torch.full((B,), nan, device=d)
    d_ge = torch.full((1,), nan, device=d)
    p = R.native.ptr
    if batch_global is None:
        rc = lib.rnb_loss_rnb(p(color), p(rgb), p(mask), p(ws), p(ge), L, B, Cd, igr_w, mask_w, p(loss), p(parts),
                              p(d_color), p(d_ws), p(d_ge), None)
    else:
        bg = torch.tensor(batch_global, dtype=torch.float32, device=d)
        rc = lib.rnb_loss_rnb_shard(p(color), p(rgb), p(mask), p(ws), p(ge), L, B, Cd, igr_w, mask_w, p(bg), eik_share,
                                    p(loss), p(parts), p(d_color), p(d_ws), p(d_ge), None)
    R.native.check(rc)
    torch.cuda.synchronize()
    out = {"loss": loss[0].cpu(), "d_color": d_color.cpu(), "d_ws": d_ws.cpu(), "d_ge": d_ge[0].cpu()}
    out.update({k: parts[i].cpu() for i, k in enumerate(PARTS)})
    return out


def _check_loss(tag, got, r64, r32, skip=()):
    worst = 0.0
    for k in ("loss",) + PARTS + ("d_color", "d_ws", "d_ge"):
        if k not in skip:
            worst = max(worst, _rule(tag, k, got[k], r64[k], r32[k]))
    return worst


def _refs(inp, mask_w, **kw):
    return (T.loss_ref_run(inp, T.IGR_W, mask_w, torch.float64, **kw), T.loss_ref_run(inp, T.IGR_W, mask_w, torch.float32, **kw))


@pytest.mark.parametrize("shape", T.LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_kernel_shapes_and_edges(R, shape):
    """every edge value of weight_sum under both masks, the six mask values, exact zeros and -0.0 of the L1 term, at sizes
    that wrap the 1024-thread strided loops and exercise (i / Cd) % B"""
    B, L, Cd = shape
    inp = T.loss_inputs(B, L, Cd, seed=B + L)
    r64, r32 = _refs(inp, T.MASK_W)
    got = _loss_direct(R, inp, T.IGR_W, T.MASK_W)
    tag = f"loss {B}x{L}x{Cd}"
    _check_loss(tag, got, r64, r32)
    # exact zeros: clip's sub-gradient outside [lo, hi], the sign gradient where color == rgb or the ray is masked out
    assert bool((got["d_ws"][r64["d_ws"] == 0] == 0).all()), f"{tag}: d_weight_sum must be exactly 0 outside the clip range"
    assert bool((got["d_ws"][r64["d_ws"] != 0] != 0).all()), f"{tag}: clip's sub-gradient is inclusive"
    assert bool((got["d_color"][r64["d_color"] == 0] == 0).all()), f"{tag}: the sign gradient must be exactly 0"
    assert bool((got["d_color"][r64["d_color"] != 0] != 0).all())


@pytest.mark.parametrize("mode", ["zeros", "ones", "mask_weight_0"])
def test_loss_kernel_mask_extremes(R, mode):
    B, L, Cd = 65, 2, 3
    mask_w = 0.0 if mode == "mask_weight_0" else T.MASK_W
    inp = T.loss_inputs(B, L, Cd, seed=1, mask_mode="mixed" if mode == "mask_weight_0" else mode)
    r64, r32 = _refs(inp, mask_w)
    got = _loss_direct(R, inp, T.IGR_W, mask_w)
    _check_loss(f"loss mask {mode}", got, r64, r32)
    if mode == "zeros":       # mask_sum = 1e-5
        assert float(got["color_loss"]) == 0.0 and bool((got["d_color"] == 0).all())
    if mode == "mask_weight_0":     # the mask is ignored
        assert bool((got["d_ws"] == 0).all())
        ones = _loss_direct(R, T.loss_inputs(B, L, Cd, seed=1, mask_mode="ones"), T.IGR_W, mask_w)
        assert torch.equal(ones["d_color"], got["d_color"]) and torch.equal(ones["color_loss"], got["color_loss"])


@pytest.mark.parametrize("special", ["nan_ws", "inf_color"])
def test_loss_kernel_non_finite_inputs(R, special):
    """a NaN weight_sum poisons the mask loss, a +inf colour entry the colour loss, and the total; everything else is
    held to the rule, the other rays' gradients included"""
    B, L, Cd = 65, 2, 3
    inp = T.loss_inputs(B, L, Cd, seed=2, special=special)
    r64, r32 = _refs(inp, T.MASK_W)
    got = _loss_direct(R, inp, T.IGR_W, T.MASK_W)
    bad = [k for k in ("loss",) + PARTS if not bool(torch.isfinite(r64[k]))]
    assert bad == (["loss", "mask_loss"] if special == "nan_ws" else ["loss", "color_loss"])
    for k in bad:
        g, r = float(got[k]), float(r64[k])
        assert (g != g) == (r != r) and (r != r or g == r), f"{special}: {k} is {g} on the device, {r} in fp64"
    _check_loss(f"loss {special}", got, r64, r32, skip=bad)       # d_color, d_ws, d_ge: every ray, the poisoned one included
    if special == "nan_ws":       # torch autograd through clip: no gradient for a NaN
        assert float(r64["d_ws"][B - 1]) == 0.0 and float(got["d_ws"][B - 1]) == 0.0


def test_loss_wrapper_backward_and_layouts(R):
    """R.rnb_loss: an upstream gradient other than 1, a second backward, and the [B, 3] / fp64 / bool / non-contiguous
    inputs, which give the contiguous fp32 call's numbers bit for bit"""
    d = device()
    B, L, Cd = 65, 2, 3
    inp = T.loss_inputs(B, L, Cd, seed=7)
    color, rgb, mask, ws, ge = inp
    r64, r32 = _refs(inp, T.MASK_W, upstream=1.7)

    def run(color, rgb, mask, ws, ge, twice=False):
        leaves = [color.to(d).requires_grad_(True), ws.to(d).requires_grad_(True), ge.to(d).requires_grad_(True)]
        loss, parts = R.rnb_loss({"color_fine": leaves[0], "weight_sum": leaves[1], "gradient_error": leaves[2]},
                                 rgb.to(d), mask.to(d), igr_weight=T.IGR_W, mask_weight=T.MASK_W)
        (loss * 1.7).backward(retain_graph=twice)
        if twice:
            with pytest.raises(RuntimeError, match="backward called twice"):
                loss.backward()
        out = {"loss": loss.detach().cpu(), "d_color": leaves[0].grad.cpu(), "d_ws": leaves[1].grad.cpu(),
               "d_ge": leaves[2].grad.cpu()}
        out.update({k: parts[k].cpu() for k in PARTS})
        return out

    base = run(color, rgb, mask.reshape(-1, 1), ws.reshape(-1, 1), ge, twice=True)
    base["d_ws"] = base["d_ws"].reshape(-1)
    _check_loss("loss wrapper x1.7", base, r64, r32)
    direct = _loss_direct(R, inp, T.IGR_W, T.MASK_W)
    for k in ("loss",) + PARTS:
        assert torch.equal(base[k], direct[k]), k

    def same(tag, got):
        for k in base:
            a = got[k].float().reshape(base[k].shape)
            assert torch.equal(a, base[k]), f"{tag}: {k} differs from the contiguous fp32 call"

    # fp64 inputs and a bool mask (mask values {0, 1}: the same selection as mask > 0.5)
    mask01 = (mask > 0.5)
    base01 = run(color, rgb, mask01.float().reshape(-1, 1), ws.reshape(-1, 1), ge)
    got = run(color.double(), rgb.double(), mask01.reshape(-1, 1), ws.double().reshape(-1, 1), ge.double())
    assert got["d_color"].dtype == torch.float64
    for k in base01:
        assert torch.equal(got[k].float().reshape(base01[k].shape), base01[k]), f"fp64 + bool: {k}"
    assert torch.equal(base01["d_color"], base["d_color"])        # (mask > 0.5 of the six values is that selection)
    # a non-contiguous color_fine: [B, L, Cd] storage seen as [L, B, Cd]
    nc = color.permute(1, 0, 2).contiguous().to(d).permute(1, 0, 2)
    assert not nc.is_contiguous()
    same("non-contiguous", run(nc, rgb, mask.reshape(-1, 1), ws.reshape(-1, 1), ge))
    # the single-light layout [B, 3] against [1, B, 3]
    one = run(color[:1], rgb[:1], mask.reshape(-1, 1), ws.reshape(-1, 1), ge)
    flat = run(color[0], rgb[0], mask.reshape(-1, 1), ws.reshape(-1, 1), ge)
    assert flat["d_color"].shape == (B, Cd)
    for k in one:
        assert torch.equal(flat[k].reshape(one[k].shape), one[k]), f"[B, 3]: {k}"


@pytest.mark.parametrize("mask_w", [T.MASK_W, 0.0], ids=["mask_weight", "mask_weight_0"])
def test_loss_shard_form_in_one_process(R, mask_w):
    """rnb_loss_rnb_shard on shards of 37, 1 and 90 rays with the whole batch's counts: the gradients are the whole-batch
    call's bit for bit (both forms normalise by the same fp32 numbers: the contract of the exact data-parallel mode), the
    values are additive shares"""
    inp = T.loss_inputs(128, 2, 3, seed=128)
    color, rgb, mask, ws, ge = inp
    count = float((mask > 0.5).sum()) if mask_w > 0 else 128.0
    whole = _loss_direct(R, inp, T.IGR_W, mask_w)
    r64, r32 = _refs(inp, mask_w)
    _check_loss(f"loss whole 128 mw {mask_w}", whole, r64, r32)
    tot = {k: 0.0 for k in ("loss",) + PARTS}
    dc, dw, b0 = [], [], 0
    for n in T.LOSS_SHARDS:
        sl = slice(b0, b0 + n)
        sh = (color[:, sl], rgb[:, sl], mask[sl], ws[sl], ge)
        kw = dict(batch_global=(count, 128.0), eik_share=1.0 / 3.0)
        got = _loss_direct(R, sh, T.IGR_W, mask_w, **kw)
        s64, s32 = _refs(sh, mask_w, **kw)
        # (d_gradient_error stays igr_weight in the shard form: the renderer's backward owns the eikonal share)
        _check_loss(f"loss shard {n} mw {mask_w}", got, s64, s32, skip=("d_ge",))
        for k in tot:
            tot[k] += float(got[k].double())
        dc.append(got["d_color"])
        dw.append(got["d_ws"])
        b0 += n
    assert torch.equal(torch.cat(dc, 1), whole["d_color"]), "shard d_color_fine != whole batch, bit for bit"
    assert torch.equal(torch.cat(dw), whole["d_ws"]), "shard d_weight_sum != whole batch, bit for bit"
    for k in tot:
        _rule(f"loss shards summed mw {mask_w}", k, torch.tensor(tot[k]), r64[k], r32[k])


# ----------------------------------------------------------------------------------------------------------------- Adam
SENTINEL = -123456.0
TAIL = 64


def _adam_direct(R, p, g, m, v, n, lr, betas, eps, wd, step):
    lib = R.native.load()
    ptr = R.native.ptr
    return lib.rnb_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), n, lr, betas[0], betas[1], eps, wd, step, None)


def _check_adam(tag, dev, r64, r32, betas):
    """dev, r64, r32: (p, m, v) of one tensor.  Parameters by the value rule; moments by relative L2 against
    max(K_OUT x the fp32 reference's own error, 4 * 2^-24 / (1 - beta)) (train_ops_ref.adam_moment_floor)."""
    worst = _rule(tag, "p", dev[0], r64[0], r32[0])
    for name, k, beta in (("exp_avg", 1, betas[0]), ("exp_avg_sq", 2, betas[1])):
        e_dev, e_ref = T.rel_l2(dev[k].cpu(), r64[k]), T.rel_l2(r32[k], r64[k])
        bound = max(P.ref_term(e_ref), T.adam_moment_floor(beta))
        print(f"TRAINOPS {tag} {name}: relL2 {e_dev:.3e}  fp32 ref {e_ref:.3e}  bound {bound:.3e}  ratio {e_dev / bound:.3f}")
        assert e_dev <= bound, f"{tag} {name}: relL2 {e_dev:.3e} > {bound:.3e} (fp32 reference: {e_ref:.3e})"
        worst = max(worst, e_dev / bound)
    return worst


@pytest.mark.parametrize("setting", list(T.ADAM_SETTINGS))
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65536 + 3])
def test_adam_step_direct(R, n, setting):
    """three rnb_adam_step calls on buffers 64 floats longer than n: the tails stay untouched, the values follow the
    references; then a step with lr = 0"""
    betas, eps, wd, _ = T.ADAM_SETTINGS[setting]
    d = device()
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    grads = [(torch.randn(n, generator=gen) + 0.3) * (10.0 if it == 1 else 1e-3) for it in range(3)]
    lrs = [T.adam_lr(it, 3) for it in range(3)]

    def padded(x):
        return torch.cat([x, torch.full((TAIL,), SENTINEL)]).to(d)

    p, m, v = padded(p0), padded(torch.zeros(n)), padded(torch.zeros(n))
    for it in range(3):
        assert _adam_direct(R, p, padded(grads[it]), m, v, n, lrs[it], betas, eps, wd, it + 1) == 0
    torch.cuda.synchronize()
    for name, t in (("p", p), ("exp_avg", m), ("exp_avg_sq", v)):
        assert bool((t[n:] == SENTINEL).all()), f"n {n}: {name} written past n"
    r64 = T.adam_ref(p0, grads, lrs, betas, eps, wd, torch.float64)
    r32 = T.adam_ref(p0, grads, lrs, betas, eps, wd, torch.float32)
    _check_adam(f"adam direct n {n} {setting}", (p[:n], m[:n], v[:n]), r64, r32, betas)
    # lr = 0: p unchanged bit for bit, the moments still move
    before = [t.clone() for t in (p, m, v)]
    assert _adam_direct(R, p, padded(grads[0]), m, v, n, 0.0, betas, eps, wd, 4) == 0
    torch.cuda.synchronize()
    assert torch.equal(p, before[0])
    assert not torch.equal(m[:n], before[1][:n]) and not torch.equal(v[:n], before[2][:n])
    assert bool((m[n:] == SENTINEL).all()) and bool((v[n:] == SENTINEL).all())


def test_adam_step_argument_checks(R):
    d = device()
    bufs = [torch.full((TAIL,), SENTINEL, device=d) for _ in range(4)]
    hp = (1e-3, (0.9, 0.999), 1e-8, 0.0)
    assert _adam_direct(R, bufs[0], bufs[1], bufs[2], bufs[3], 0, *hp, 1) == 0             # n = 0: nothing to do
    assert _adam_direct(R, bufs[0], bufs[1], bufs[2], bufs[3], 8, *hp, 0) == RNB_E_INVALID  # step counts from 1
    assert _adam_direct(R, bufs[0], bufs[1], bufs[2], bufs[3], -1, *hp, 1) == RNB_E_INVALID
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in bufs)


def _flat_adam(R, p0, setting, lr=T.ADAM_BASE_LR):
    betas, eps, wd, _ = T.ADAM_SETTINGS[setting]
    ps = [torch.nn.Parameter(r.clone().to(device())) for r in p0]
    return ps, R.FlatAdam(ps, lr=lr, betas=betas, eps=eps, weight_decay=wd)


def _flat_steps(opt, ps, seq_dev, lrs):
    for g, lr in zip(seq_dev, lrs):
        for p, gi in zip(ps, g):
            p.grad = gi
        opt.param_groups[0]["lr"] = lr
        opt.step()
    torch.cuda.synchronize()


def _flat_state(opt, ps):
    k, n = len(ps), ps[0].numel()
    return (torch.stack([p.detach() for p in ps]).cpu(), opt.exp_avg.view(k, n).cpu(), opt.exp_avg_sq.view(k, n).cpu())


@pytest.mark.parametrize("setting", list(T.ADAM_SETTINGS))
def test_flat_adam_long_run(R, setting):
    """2,000 (500) steps on one tensor per gradient scale 1e-12 .. 1e4 against the fp64 textbook loop, calibrated by
    torch.optim.Adam in fp32 on the CPU.  Parameters by absolute error: with gradients of 1e-12 against eps 1e-8 the
    per-step update is below the fp32 spacing of a parameter of size 1 and is lost in every fp32 run."""
    betas, eps, wd, steps = T.ADAM_SETTINGS[setting]
    (p64, m64, v64), (p32, m32, v32) = T.adam_long_refs(setting)
    p0 = T.adam_params0()
    ps, opt = _flat_adam(R, p0, setting)
    _flat_steps(opt, ps, T.adam_grad_sequence(steps).to(device()), [T.adam_lr(it, steps) for it in range(steps)])
    assert opt.step_count == steps
    p, m, v = _flat_state(opt, ps)
    for k, scale in enumerate(T.ADAM_SCALES):
        _check_adam(f"adam long {setting} g {scale:g}", (p[k], m[k], v[k]), (p64[k], m64[k], v64[k]),
                    (p32[k], m32[k], v32[k]), betas)
        head = slice(0, T.ADAM_ZERO_HEAD)
        if wd == 0.0:     # a gradient of exactly 0 never moves its parameter
            assert torch.equal(p[k, head], p0[k, head]), f"{setting} g {scale:g}: a zero-gradient parameter moved"
            assert bool((m[k, head] == 0).all()) and bool((v[k, head] == 0).all())
        else:
            assert not torch.equal(p[k, head], p0[k, head])


RESUME = "decay"


def test_flat_adam_resume(R):
    """a run resumed from state_dict() continues like the original bit for bit; the same state continues inside
    torch.optim.Adam, and a torch.optim.Adam state continues inside FlatAdam, within the rules of the long run"""
    betas, eps, wd, _ = T.ADAM_SETTINGS[RESUME]
    d = device()
    steps = 20
    seq = T.adam_grad_sequence(steps)
    seq_dev = seq.to(d)
    lrs = [T.adam_lr(it, steps) for it in range(steps)]
    p0 = T.adam_params0()
    flat = lambda x: x.reshape(-1)
    r64 = T.adam_ref(flat(p0), seq.reshape(steps, -1), lrs, betas, eps, wd, torch.float64)
    r32 = tuple(flat(t) for t in T.torch_adam_run(p0, seq, lrs, betas, eps, wd, torch.float32)[:3])
    # A: 20 steps
    ps_a, opt_a = _flat_adam(R, p0, RESUME)
    _flat_steps(opt_a, ps_a, seq_dev, lrs)
    a = _flat_state(opt_a, ps_a)
    _check_adam("adam resume A", tuple(flat(t) for t in a), r64, r32, betas)
    # B: 10 steps, state_dict() into a new FlatAdam over a copy of B's parameters, steps 11 .. 20
    ps_b, opt_b = _flat_adam(R, p0, RESUME)
    _flat_steps(opt_b, ps_b, seq_dev[:10], lrs[:10])
    sd = opt_b.state_dict()
    mid = [p.detach().clone() for p in ps_b]
    ps_c = [torch.nn.Parameter(t.clone()) for t in mid]
    opt_c = R.FlatAdam(ps_c, lr=1.0)              # every hyper-parameter comes from the state dict
    opt_c.load_state_dict(sd)
    assert opt_c.step_count == 10
    _flat_steps(opt_c, ps_c, seq_dev[10:], lrs[10:])
    c = _flat_state(opt_c, ps_c)
    assert opt_c.step_count == opt_a.step_count == 20
    for name, x, y in zip(("p", "exp_avg", "exp_avg_sq"), c, a):
        assert torch.equal(x, y), f"resumed FlatAdam: {name} differs from the uninterrupted run"
    # the same state dict inside torch.optim.Adam (CPU, fp32), steps 11 .. 20
    cpu_sd = {"state": {i: {k: v.cpu() for k, v in st.items()} for i, st in sd["state"].items()},
              "param_groups": sd["param_groups"]}
    t = T.torch_adam_run(torch.stack([x.cpu() for x in mid]), seq[10:], lrs[10:], betas, eps, wd, torch.float32,
                         state_dict=cpu_sd)
    assert int(float(t[3].state_dict()["state"][0]["step"])) == 20
    _check_adam("adam resume FlatAdam -> torch", tuple(flat(x) for x in t[:3]), r64, r32, betas)
    # the opposite direction: torch.optim.Adam for 10 steps, its state inside FlatAdam for steps 11 .. 20
    tp, _, _, topt = T.torch_adam_run(p0, seq[:10], lrs[:10], betas, eps, wd, torch.float32)
    ps_e = [torch.nn.Parameter(r.clone().to(d)) for r in tp]
    opt_e = R.FlatAdam(ps_e, lr=1.0)
    opt_e.load_state_dict(topt.state_dict())
    assert opt_e.step_count == 10 and opt_e.param_groups[0]["weight_decay"] == wd
    _flat_steps(opt_e, ps_e, seq_dev[10:], lrs[10:])
    _check_adam("adam resume torch -> FlatAdam", tuple(flat(x) for x in _flat_state(opt_e, ps_e)), r64, r32, betas)
    # amsgrad keeps a third moment FlatAdam does not have
    bad = topt.state_dict()
    bad["param_groups"][0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        R.FlatAdam([torch.nn.Parameter(r.clone().to(d)) for r in tp]).load_state_dict(bad)
