"""Opt-in autograd of the direct network calls (SDFNetwork / RenderingNetwork.set_autograd) against the fp64 oracle.

Losses on sdf_network(x), .gradient(x) (the eikonal term: the reference's create_graph=True double backward) and
color_network(p, n, n, f) are differentiated natively (rnb_sdf_backward / rnb_color_backward + rnb_weightnorm_bwd) and
compared with torch autograd through oracle/rnb_oracle.py in fp64, with the calibrated rule of tests/parity.py: outputs
by check_value (the fp32 oracle's own max error calibrates), gradients by check_grad (rel-L2 of fp32 vs fp64 calibrates).  States
are shape_matrix.live_params, so the encoding's columns carry weight."""
import pytest
import torch

from oracle import rnb_oracle as O
from tests.field_autograd_util import build as _build, check_grad_or_zero as _check_grad, compare_leaves as _compare_leaves, \
    mesh_texture as _mesh_texture, native_leaf_grads as _native_leaf_grads, oracle as _oracle, oracle_normal as _oracle_normal, \
    weights as _weights, zero_grads as _zero
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import ALBEDO_H2_CLASSES, device, profile_classes
from tests.parity import check_value, rel_l2
from tests.shape_matrix import points

pytestmark = pytest.mark.gpu

SDF_SHAPES = ["default_64x64", "no_skip", "skip1", "skip7", "scale3", "multires0", "no_weight_norm", "feat128", "w100"]
COLOR_SHAPES = ["default_64x64", "mview0", "albedo_nl1", "feat128"]
SIZES = [1, 63, 4097]
FUSED_CLASSES = {"R_sweep", "FB_sweep", "RA_sweep", "dW(x3: 256x256 + narrow jobs)"}


# ------------------------------------------------------------------------------------------------------- cases 1 and 2
@pytest.mark.parametrize("name", SDF_SHAPES)
def test_sdf_feature_loss_and_eikonal_against_fp64(R, name):
    shape, p, sdf, col, ren = _build(R, name)
    conf = shape.mc.sdf
    F = conf.d_out - 1
    for n in SIZES + ([100_000] if name == "default_64x64" else []):
        x0 = points(n, seed=n)
        w, W = _weights(n, 1, 1), _weights(n, F, 2)
        # case 1: (w sdf).sum() + (W o feat).sum()
        loss1 = lambda q, x: (lambda o: (o, (w.to(o) * o[:, :1]).sum() + (W.to(o) * o[:, 1:]).sum()))(O.sdf_forward(q, conf, x))
        o64, g64, (x64,) = _oracle(p, "sdf.", [x0], loss1, torch.float64)
        o32, g32, (x32,) = _oracle(p, "sdf.", [x0], loss1, torch.float32)
        _zero(sdf)
        x = x0.to(device()).requires_grad_(True)
        out = sdf(x)
        assert out.grad_fn is not None and out.shape == (n, conf.d_out)
        check_value(f"{name} n={n} forward", out.detach(), o64, o32)
        ((w.to(device()) * out[:, :1]).sum() + (W.to(device()) * out[:, 1:]).sum()).backward()
        _compare_leaves(_native_leaf_grads(sdf, "sdf"), g64, g32, f"{name} n={n} case1")
        _check_grad(x.grad, x64, x32, f"{name} n={n} case1 x.grad")
        # case 2: the eikonal loss on gradient(x) (the Hessian term in x.grad)
        loss2 = lambda q, x: (lambda g: (g, ((g.norm(dim=-1) - 1) ** 2).mean()))(_oracle_normal(q, conf, x))
        n64, g64, (x64,) = _oracle(p, "sdf.", [x0], loss2, torch.float64)
        n32, g32, (x32,) = _oracle(p, "sdf.", [x0], loss2, torch.float32)
        _zero(sdf)
        x = x0.to(device()).requires_grad_(True)
        g = sdf.gradient(x)
        assert g.shape == (n, 1, 3) and g.grad_fn is not None
        check_value(f"{name} n={n} gradient", g.detach().reshape(n, 3), n64, n32)
        ((g.norm(dim=-1) - 1) ** 2).mean().backward()
        _compare_leaves(_native_leaf_grads(sdf, "sdf"), g64, g32, f"{name} n={n} eikonal")
        _check_grad(x.grad, x64, x32, f"{name} n={n} eikonal x.grad")
        # sdf(): the sdf column alone, parameters only (x does not require grad: no x adjoint work)
        _zero(sdf)
        xs = x0.to(device())
        s = sdf.sdf(xs)
        (w.to(device()) * s).sum().backward()
        assert xs.grad is None and sdf.lin0.bias.grad is not None


# ------------------------------------------------------------------------------------------------------- case 3
@pytest.mark.parametrize("name", COLOR_SHAPES)
def test_color_loss_against_fp64(R, name):
    shape, p, sdf, col, ren = _build(R, name)
    cc = shape.mc.color
    for n in SIZES:
        p0 = points(n, seed=n + 7)
        nr0 = torch.nn.functional.normalize(_weights(n, 3, 3), dim=-1)
        f0 = 0.5 * _weights(n, cc.d_feature, 4)
        Wc = _weights(n, cc.d_out, 5)
        loss = lambda q, pp, nn_, ff: (lambda a: (a, (Wc.to(a) * a).sum()))(O.color_forward(q, cc, pp, nn_, nn_, ff))
        a64, g64, i64 = _oracle(p, "color.", [p0, nr0, f0], loss, torch.float64)
        a32, g32, i32 = _oracle(p, "color.", [p0, nr0, f0], loss, torch.float32)
        _zero(col)
        pp, nn_, ff = (t.to(device()).requires_grad_(True) for t in (p0, nr0, f0))
        vd = nr0.to(device()).requires_grad_(True)
        a = col(pp, nn_, vd, ff)
        assert a.grad_fn is not None
        check_value(f"{name} n={n} albedo", a.detach(), a64, a32)
        (Wc.to(device()) * a).sum().backward()
        _compare_leaves(_native_leaf_grads(col, "color"), g64, g32, f"{name} n={n} color")
        for t, r64, r32, what in zip((pp, nn_, ff), i64, i32, ("points", "normals", "feats")):
            _check_grad(t.grad, r64, r32, f"{name} n={n} {what}.grad")
        assert vd.grad is None


# ------------------------------------------------------------------------------------------------------- case 4
@pytest.mark.parametrize("name", ["default_64x64", "mview0"])
def test_validate_mesh_texture_sequence(R, name):
    shape, p, sdf, col, ren = _build(R, name)
    sc, cc = shape.mc.sdf, shape.mc.color
    lib = R.native.load()
    for n in SIZES + ([4096, 100_000] if name == "default_64x64" else []):
        v0 = points(n, seed=n + 11)
        with torch.no_grad():
            ref = _mesh_texture(sdf, col, v0.to(device()))
        Wa = _weights(n, cc.d_out, 6)

        def chain(q, v):
            nrm = _oracle_normal(q, sc, v)
            a = O.color_forward(q, cc, v, nrm, nrm, O.sdf_forward(q, sc, v)[:, 1:])
            return a, (Wa.to(a) * a).sum()
        a64, g64, _ = _oracle(p, "", [v0], chain, torch.float64)
        a32, g32, _ = _oracle(p, "", [v0], chain, torch.float32)
        _zero(sdf, col)
        profile = name == "default_64x64" and n == 4096   # (a multiple of 32 points: the staged x3 weight-gradient jobs)
        if profile:
            lib.rnb_profile_enable(1)
        try:
            alb = _mesh_texture(sdf, col, v0.to(device()))
            assert alb.grad_fn is not None
            check_value(f"{name} n={n} texture", alb.detach(), a64, a32)
            check_value(f"{name} n={n} texture (no_grad)", ref, a64, a32)
            (Wa.to(device()) * alb).sum().backward()
            if profile:
                torch.cuda.synchronize()
                classes = profile_classes(R)
                assert FUSED_CLASSES <= classes, f"fused sweeps missing: {sorted(FUSED_CLASSES - classes)}"
                assert ALBEDO_H2_CLASSES <= classes, "the fused albedo sweeps did not run"
        finally:
            lib.rnb_profile_enable(0)
        mine = _native_leaf_grads(sdf, "sdf")
        mine.update(_native_leaf_grads(col, "color"))
        g64 = {k: v for k, v in g64.items() if k.startswith(("sdf.", "color."))}
        _compare_leaves(mine, g64, g32, f"{name} n={n} texture")
        # the SDF leaves get gradient through the feature AND the normal: the feature head's rows and lin0 both move
        assert float(sdf.lin0.bias.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------- case 5
def test_render_loss_and_eikonal_accumulate(R):
    shape, p, sdf, col, ren = _build(R, "default_64x64")
    b = {k: v.to(device()) for k, v in O.synthetic_batch(64, seed=3, step=1).items()}
    x0 = points(4097, seed=5).to(device())

    def render_loss():
        out = ren.render_rnb(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=1.0,
                             t_rand=b["t_rand"])
        loss, _ = R.rnb_loss(out, b["true_rgb"], b["mask"])
        return loss

    def eik():
        return ((sdf.gradient(x0).norm(dim=-1) - 1) ** 2).mean()

    nets = (sdf, col, ren.deviation_network)
    grads = []
    for fn in (render_loss, eik, lambda: render_loss() + eik()):
        _zero(*nets)
        fn().backward()
        grads.append({k: v.grad.clone() for k, v in sdf.named_parameters()})
    for k in grads[0]:
        want = grads[0][k] + grads[1][k]
        assert rel_l2(grads[2][k], want) <= 1e-5, f"{k}: render + eikonal in one backward != the sum of the two"
    assert float(grads[1]["lin0.bias"].abs().max()) > 0 and float(grads[0]["lin0.bias"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------- cases 6, 7, 8
def test_adjoint_scale_determinism_and_lifetime(R):
    shape, p, sdf, col, ren = _build(R, "default_64x64")
    n = 4096   # (a multiple of the weight-gradient chunk: every reduction of the default arithmetic is ordered, no atomics)
    x0 = points(n, seed=9).to(device())
    f0 = 0.5 * _weights(n, 256, 4).to(device())
    nr0 = torch.nn.functional.normalize(_weights(n, 3, 3), dim=-1).to(device())
    W, Wn, Wc = _weights(n, 257, 2).to(device()), _weights(n, 3, 8).to(device()), _weights(n, 3, 5).to(device())

    def run(scale):
        _zero(sdf, col)
        x = x0.clone().requires_grad_(True)
        ((W * sdf(x)).sum() * scale + (Wn * sdf.gradient(x).squeeze(1)).sum() * scale
         + (Wc * col(x, nr0, nr0, f0)).sum() * scale).backward()
        gs = [q.grad.clone() for q in list(sdf.parameters()) + list(col.parameters())]
        return gs + [x.grad.clone()]

    base = run(1.0)
    again = run(1.0)
    for a, b in zip(base, again):   # case 7: bit-identical
        assert torch.equal(a, b)
    for k in (40, -40):              # case 6: a loss times 2^k gives gradients times 2^k, bit for bit
        s = 2.0 ** k
        for a, b in zip(base, run(s)):
            assert torch.equal(a * s, b), f"2^{k}: gradients not scaled bit for bit"
    # case 8: the second backward and create_graph=True raise; the saved state is released by the backward
    _zero(sdf, col)
    x = x0.clone().requires_grad_(True)
    torch.cuda.synchronize()
    baseline = torch.cuda.memory_allocated()
    out = sdf(x)
    loss = (W * out).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()
    del out, loss
    a = col(x0, nr0, nr0, f0)
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad((Wc * a).sum(), list(col.parameters()), create_graph=True)
    del a
    g = sdf.gradient(x0)
    with pytest.raises(RuntimeError, match="differentiable once"):
        torch.autograd.grad(g.sum(), list(sdf.parameters()), create_graph=True)
    del g
    x.grad = None
    _zero(sdf, col)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == baseline
    # the default path stays forward-only and loud, whatever the other module's flag
    sdf.set_autograd(False)
    with pytest.raises(RuntimeError, match="forward-only"):
        sdf(x0)
    with torch.no_grad():
        assert sdf(x0).grad_fn is None
