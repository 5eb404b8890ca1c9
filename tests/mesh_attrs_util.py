"""What the mesh-attribute tests share (tests/test_gpu_mesh_attrs.py, tests/test_mesh_attrs_host.py): the three models of
tests/test_gpu_sparse_grid.py's recipe (restated here: no test imports a test), deterministic point batches with a
near-surface half, and the CPU oracle's attributes / Newton step in fp32 and fp64.  Torch on the CPU only; not a test module.

References are computed once per (model, batch) and shared: callers must not modify what they get."""
import numpy as np
import torch

from oracle import rnb_oracle as O

LO, HI = torch.tensor([-1.01, -1.01, -1.01]), torch.tensor([1.01, 1.01, 1.01])
SURFACE_BAND = 0.02     # the near-surface half of a batch lies within this distance of the zero level set


def model_params(which):
    """(ModelConf, named parameters) of "sharp" / "sharp_bf16" (the trained full_main_sharp fixture: fused route, bf16: the
    bf16 route) and "tiny" (64-wide, seed 3: the per-layer route)"""
    if which in ("sharp", "sharp_bf16"):
        from tests.golden_util import Golden
        g = Golden("full_main_sharp")
        return g.mc, g.params()
    assert which == "tiny", which
    mc = O.ModelConf(sdf=O.SDFConf(d_out=65, d_hidden=64), color=O.ColorConf(d_feature=64, d_hidden=64),
                     render=O.RenderConf(n_samples=16, n_importance=16))
    torch.manual_seed(3)
    p = O.init_params(mc)
    with torch.no_grad():
        p["dev.variance"].fill_(0.4)
    return mc, p


_MODELS, _REN, _POOL, _BATCH, _REF = {}, {}, {}, {}, {}


def model(which):
    key = "sharp" if which == "sharp_bf16" else which
    if key not in _MODELS:
        mc, p = model_params(key)
        _MODELS[key] = (mc, p, {k: v.detach().double() for k, v in p.items()})
    return _MODELS[key]


def renderer(R, which, dev):
    if which not in _REN:
        mc, p, _ = model(which)
        ren = R.build_from_named_params(mc, p, dev)[3]
        if which == "sharp_bf16":
            ren.set_variant(bf16=True)
        _REN[which] = ren
    return _REN[which]


def _surface_pool(which):
    """points ON the zero level set of the model (fp64 Newton from random starts, steps clamped to 0.1) and their unit normals"""
    key = "sharp" if which == "sharp_bf16" else which
    if key not in _POOL:
        mc, _, p64 = model(key)
        g = torch.Generator().manual_seed(11)
        x = (torch.rand(192, 3, generator=g, dtype=torch.float64) * 2 - 1) * 0.7
        for _ in range(16):
            x, _, _ = newton_step(p64, mc, x, 0.0, 0.1)
        with torch.no_grad():
            f = O.sdf_only(p64, mc.sdf, x)[:, 0]
        n = O.sdf_gradient(p64, mc.sdf, x, create_graph=False)
        keep = (f.abs() < 1e-6) & (x.abs().max(dim=1).values < 0.95)
        assert int(keep.sum()) >= 100, f"{key}: only {int(keep.sum())} starts reached the surface"
        _POOL[key] = (x[keep][:100].contiguous(), torch.nn.functional.normalize(n[keep][:100], dim=1))
    return _POOL[key]


def point_batch(which, V):
    """[V,3] fp32: V // 2 points uniform in [-1,1]^3, the rest within SURFACE_BAND of the model's surface"""
    key = ("sharp" if which == "sharp_bf16" else which, V)
    if key not in _BATCH:
        g = torch.Generator().manual_seed(1000 + V)
        n_uni = V // 2
        uni = torch.rand(n_uni, 3, generator=g, dtype=torch.float64) * 2 - 1
        xs, ns = _surface_pool(which)
        idx = torch.randint(0, xs.shape[0], (V - n_uni,), generator=g)
        off = (torch.rand(V - n_uni, 1, generator=g, dtype=torch.float64) * 2 - 1) * (0.9 * SURFACE_BAND)
        _BATCH[key] = torch.cat([uni, xs[idx] + ns[idx] * off]).float().contiguous()
    return _BATCH[key]


def attributes(p, mc, pts):
    """(sdf [V,1], gradient [V,3], albedo [V,C]) of the oracle in the dtype of p / pts: the reference's
    sdf_network(v), sdf_network.gradient(v), color_network(v, g, g, feat) (exp_runner.py:607-610)"""
    with torch.no_grad():
        out = O.sdf_forward(p, mc.sdf, pts)
    grad = O.sdf_gradient(p, mc.sdf, pts, create_graph=False).detach()
    with torch.no_grad():
        alb = O.color_forward(p, mc.color, pts, grad, grad, out[:, 1:])
    return out[:, :1].contiguous(), grad, alb


def oracle_attributes(which, pts32, tag=None):
    """{"sdf" | "gradient" | "albedo": (r64, r32)} on the fp32 points given (both runs start from the same fp32 values)"""
    key = (which, tag)
    if tag is None or key not in _REF:
        mc, p, p64 = model(which)
        pts32 = pts32.detach().cpu().float()
        r32 = attributes(p, mc, pts32)
        r64 = attributes(p64, mc, pts32.double())
        ref = {k: (a, b) for k, a, b in zip(("sdf", "gradient", "albedo"), r64, r32)}
        if tag is None:
            return ref
        _REF[key] = ref
    return _REF[key]


def newton_step(p, mc, x, level, max_step):
    """One step p <- p - t g, t = (sdf - level) / |g|^2, displacement |t| |g| clamped to max_step, in the dtype of x.
    Returns (new points, sdf, gradient)."""
    with torch.no_grad():
        f = O.sdf_only(p, mc.sdf, x)
    g = O.sdf_gradient(p, mc.sdf, x, create_graph=False).detach()
    g2 = (g * g).sum(dim=1, keepdim=True)
    t = (f - level) / g2
    disp = t.abs() * g2.sqrt()
    t = torch.where(disp > max_step, t * (max_step / disp), t)
    return x - t * g, f, g


def oracle_newton(which, pts32, level, max_step):
    """(r64, r32): the points after one step from the fp32 points given"""
    mc, p, p64 = model(which)
    pts32 = pts32.detach().cpu().float()
    return newton_step(p64, mc, pts32.double(), level, max_step)[0], newton_step(p, mc, pts32, level, max_step)[0]


def quantize_rgb(albedo):
    """the kernel's colour rule on a CPU fp32 tensor [V,3]: uint8 rint(255 clip(albedo[:, [2,1,0]], 0, 1))"""
    a = albedo.detach().cpu().float()[:, [2, 1, 0]]
    return torch.round(255.0 * a.clamp(0.0, 1.0)).to(torch.uint8)


def host_points(grid_vertices, res):
    """extract_geometry's rescaling of grid-index vertices (numpy, float64) followed by torch's conversion to float32"""
    v = np.asarray(grid_vertices, dtype=np.float64)
    v = v / (res - 1.0) * (HI - LO).numpy()[None, :] + LO.numpy()[None, :]
    return torch.tensor(v).type(torch.float32)
