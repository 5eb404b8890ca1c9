"""What the tests of the direct network calls' autograd share (tests/test_gpu_field_autograd.py, tests/test_gpu_point_matrix.py):
the torch oracle of a loss on those calls in fp64 / fp32, and the comparison of the native leaf gradients with it by the rule of
tests/parity.py.  Not a test module: test modules import from here, never from each other."""
import torch

from oracle import rnb_oracle as O
from tests.gpu_support import device
from tests.parity import check_grad, rel_l2
from tests.shape_matrix import BY_NAME, live_params


def build(R, name):
    """the device modules of a tests/shape_matrix.py shape in its live state, autograd of the direct calls switched on"""
    shape = BY_NAME[name]
    p = live_params(shape.mc, shape.seed)
    sdf, devn, col, ren = R.build_from_named_params(shape.mc, p, device())
    sdf.set_autograd(True)
    col.set_autograd(True)
    return shape, p, sdf, col, ren


def check_grad_or_zero(got, g64, g32, what):
    """check_grad; a tensor whose fp64 gradient vanishes must be exactly zero on the device.  Returns rel / bound."""
    if float(g64.abs().max()) == 0.0:
        assert float(got.abs().max()) == 0.0, f"{what}: non-zero gradient where the oracle's is zero"
        return 0.0
    return check_grad(what, got, g64, rel_l2(g32, g64))


def oracle(p, prefix, inputs, fn, dt, dev=None):
    """(output, {leaf: grad}, [input grads]) of loss = fn(q, *xs)[1] by torch autograd in dtype dt on the device."""
    dev = device() if dev is None else dev
    q = {k: v.to(dev, dt).detach().requires_grad_(k.startswith(prefix)) for k, v in p.items()}
    xs = [t.to(dev, dt).detach().requires_grad_(True) for t in inputs]
    with torch.enable_grad():
        out, loss = fn(q, *xs)
        keys = [k for k in q if k.startswith(prefix)]
        ins = [q[k] for k in keys] + xs
        gs = torch.autograd.grad(loss, ins, allow_unused=True)
    gs = [torch.zeros_like(t) if g is None else g for g, t in zip(gs, ins)]   # (e.g. the sdf bias in an eikonal loss)
    return out.detach(), dict(zip(keys, gs[:len(keys)])), list(gs[len(keys):])


def oracle_normal(q, conf, x):
    """d sdf / d x with a graph (models/fields.py:114-127, create_graph=True), differentiable in x as well."""
    y = O.sdf_only(q, conf, x)
    (g,) = torch.autograd.grad(y, x, torch.ones_like(y), create_graph=True)
    return g


def native_leaf_grads(net, prefix):
    return {f"{prefix}.{k}": v.grad for k, v in net.named_parameters()}


def zero_grads(*nets):
    for net in nets:
        for q in net.parameters():
            q.grad = None


def compare_leaves(mine, g64, g32, tag):
    """every leaf of the oracle against the native one, one by one.  Returns {leaf: rel / bound}."""
    assert set(mine) == set(g64), f"{tag}: leaves {sorted(set(mine) ^ set(g64))}"
    ratios = {}
    for k in g64:
        assert mine[k] is not None, f"{tag} {k}: no gradient"
        ratios[k] = check_grad_or_zero(mine[k], g64[k], g32[k], f"{tag} {k}")
    return ratios


def weights(n, width, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, width, generator=g)


def mesh_texture(sdf, col, v):
    """Runner.validate_mesh_texture's three calls (exp_runner.py:584-615)."""
    feats = sdf.sdf_hidden_appearance(v)[:, 1:]
    normals = sdf.gradient(v).squeeze(1)
    return col(v, normals, normals, feats)
