"""The network shapes the library accepts, beyond the shipped one (confs/wmask_rnb.conf), with the path each one must take.

A plain module shared by tests/test_shape_paths.py (host: the table against the library's own layout queries) and
tests/test_gpu_shapes.py (device: every entry against the fp64 oracle).  The host test pins the table, so the GPU tests
cannot end up testing a generic path under a fused label.

Per entry:
  path      "x2h": the fused 256-wide sweeps (fused.hip, fused_bwd.hip, the x3 weight gradients) in the default
            arithmetic; "generic": the per-layer GEMMs (layers.hip, gemm.hip.h, dw.hip).  fused.hip fused_supported decides: hidden
            width 256, pe <= FEP = 40, feature width 225..256 (a 256-row feature head, or none).
  bf16      RNB_VARIANT_BF16 accepts the shape: a fused shape with Ep = 64 and no skip connection at layer 1
            (make_layout rejects it otherwise).
  color_h2  the albedo network runs as the two fused x2h sweeps of color_h2.hip (color_h2_supported: F = 256, two hidden
            layers 256 wide, Ep = 64, Cinp - F = 64); otherwise as layer GEMMs behind the fused SDF sweeps.
  mv        sweep_mv.hip sweep_mv_supported: Ep = 64, 2..8 hidden layers, every hidden layer >= 192 outputs, feature
            width a multiple of 4 with a 256-row head.  Only forward-only sweeps (point queries, sampling) take it, and
            only with RNB_VARIANT_REG_TILE.
  render    the albedo network has 3 outputs, so a render (and a train step) is defined; d_out 1 and 4 are point-wise only.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, replace

import torch

from oracle import rnb_oracle as O

# 64 rays x (n_samples + n_importance) in the end-to-end step; one fused shape runs at 64 + 64
STEP_RENDER = O.RenderConf(n_samples=16, n_importance=16, up_sample_steps=4)
WIDE_RENDER = O.RenderConf(n_samples=64, n_importance=64, up_sample_steps=4)


@dataclass(frozen=True)
class Shape:
    name: str
    mc: O.ModelConf
    path: str
    bf16: bool
    color_h2: bool
    mv: bool
    why: str
    seed: int = 4      # live_params seed: a state whose step batch renders a surface (_assert_has_surface)

    @property
    def render(self) -> bool:
        return self.mc.color.d_out == 3

    @property
    def fused(self) -> bool:
        return self.path == "x2h"

    @property
    def pe(self) -> int:
        return 3 * (1 + 2 * self.mc.sdf.multires)

    def __repr__(self):   # (pytest ids)
        return self.name


def _mc(F=256, render=STEP_RENDER, color=None, **sdf):
    c = dict(d_feature=F)
    c.update(color or {})
    return O.ModelConf(sdf=O.SDFConf(d_out=F + 1, **sdf), color=O.ColorConf(**c), render=render)


def _s(name, mc, path, bf16, color_h2, mv, why, **kw):
    return Shape(name, mc, path, bf16, color_h2, mv, why, **kw)


SHAPES = [
    # ---- fused SDF sweeps, 256 wide ------------------------------------------------------------------------------------
    _s("default_64x64", _mc(render=WIDE_RENDER), "x2h", True, True, True,
       "the shipped shape at 64 + 64 samples: the reference point of every other entry"),
    _s("no_skip", _mc(skip_in=()), "x2h", True, True, True, "no skip connection: no PE tail on any layer"),
    _s("skip1", _mc(skip_in=(1,)), "x2h", False, True, True, "skip at layer 1: the PE tail is layer 0's output (n_real[0])"),
    _s("skip7", _mc(skip_in=(7,)), "x2h", True, True, True, "skip at the last hidden layer"),
    _s("nl2_skip1", _mc(n_layers=2, skip_in=(1,)), "x2h", False, True, True, "two hidden layers, the skip between them"),
    _s("nl1", _mc(n_layers=1, skip_in=()), "x2h", True, True, False, "one hidden layer: layer 0 feeds the heads directly"),
    _s("nl15", _mc(n_layers=15), "x2h", True, True, False, "15 hidden layers: the most RNB_MAX_LIN allows"),
    _s("multires0", _mc(multires=0, skip_in=()), "x2h", False, False, False,
       "no encoding: pe = 3, Ep = 32 (a padded 32-column PE tile)"),
    _s("multires4", _mc(multires=4), "x2h", False, False, False, "pe = 27, Ep = 32, skip tail of 27 columns"),
    _s("multires5", _mc(multires=5), "x2h", True, True, True, "pe = 33, Ep = 64: a part-empty second PE block"),
    _s("feat1", _mc(F=1), "generic", False, False, False,
       "feature width 1 (Fp 32): the fused FB sweep needs a 256-row feature head, so the per-layer path"),
    _s("feat128", _mc(F=128), "generic", False, False, False,
       "feature width 128 (Fp 128): the per-layer path, as feature width 1"),
    _s("feat255", _mc(F=255), "x2h", True, False, False, "feature width 255: one row short of a full tile"),
    _s("scale3", _mc(scale=3.0, bias=1.5), "x2h", True, True, True,
       "sdf_scale 3 (bias 1.5 keeps the initial sphere at radius 0.5): inv_scale in the seed, R and FB"),
    _s("no_weight_norm", replace(_mc(weight_norm=False), color=O.ColorConf(weight_norm=False)), "x2h", True, True, True,
       "plain weights on both nets: no g / v split"),
    _s("mview3", _mc(color=dict(multires_view=3)), "x2h", True, True, True,
       "multires_view 3: pev = 21, Cin = 298, Cinp - F = 64: an odd octave count for color_h2's stride-2 encode, and no "
       "octave for the fourth thread of a point in its stride-4 adjoint"),
    # ---- fused SDF sweeps, the albedo network as layer GEMMs --------------------------------------------------------------
    _s("mview0", _mc(color=dict(multires_view=0)), "x2h", True, False, True, "multires_view 0: Cin = 262, Cinp - F = 32"),
    _s("albedo_nl1", _mc(color=dict(n_layers=1)), "x2h", True, False, True, "one hidden albedo layer"),
    _s("albedo_nl3", _mc(color=dict(n_layers=3)), "x2h", True, False, True, "three hidden albedo layers"),
    _s("albedo_w128", _mc(color=dict(d_hidden=128)), "x2h", True, False, True, "albedo width 128"),
    _s("no_squeeze", _mc(color=dict(squeeze_out=False)), "x2h", True, True, True, "albedo without the output sigmoid"),
    _s("albedo_out1", _mc(color=dict(d_out=1)), "x2h", True, True, True, "one albedo output (point-wise only)"),
    _s("albedo_out4", _mc(color=dict(d_out=4)), "x2h", True, True, True, "four albedo outputs (point-wise only)"),
    # ---- per-layer GEMMs ------------------------------------------------------------------------------------------------
    _s("multires7", _mc(multires=7), "generic", False, False, False, "pe = 45 > FEP = 40: the one 256-wide generic shape"),
    _s("w100", _mc(F=37, d_hidden=100, color=dict(d_hidden=72)), "generic", False, False, False,
       "width 100 (Hp 128), feature 37, albedo 72: padded rows and columns everywhere"),
    _s("w160", _mc(F=160, d_hidden=160, color=dict(d_hidden=160)), "generic", False, False, False, "width 160 (Hp 160)"),
    _s("w288", _mc(F=64, d_hidden=288, color=dict(d_hidden=288)), "generic", False, False, False,
       "width 288: wider than the fused kernels, feature 64", seed=3),
    _s("w32", _mc(F=32, d_hidden=32, multires=3, color=dict(d_hidden=32)), "generic", False, False, False,
       "width 32, multires 3, skip 4: the skip layer has 32 - 21 = 11 outputs"),
]
BY_NAME = {s.name: s for s in SHAPES}


def _effective(p, prefix):
    return O.effective_weight(p, prefix)


def pe_columns(p, mc):
    """{name: weight columns that multiply the positional encoding's sin / cos terms} of lin0 and the skip layer."""
    sc = mc.sdf
    pe = 3 * (1 + 2 * sc.multires)
    out = {}
    if pe > 3:
        out["sdf.lin0"] = _effective(p, "sdf.lin0")[:, 3:pe]
        for s in sc.skip_in:
            w = _effective(p, f"sdf.lin{s}")
            out[f"sdf.lin{s}"] = w[:, w.shape[1] - (pe - 3):]
    return out


def live_params(mc: O.ModelConf, seed: int):
    """The geometric init of `mc` (seed `seed`) with seeded noise on every weight and bias, so that no block of any matrix
    is zero (at plain geometric init lin0's and the skip layer's PE columns are exactly zero, and the PE share of every
    Jacobian with them), and `variance` in [0.3, 0.4].  The noise is 3 % of each tensor's rms (biases: 0.003,
    weight_g: 2 %), small enough that the initial sphere keeps its surface."""
    torch.manual_seed(seed)
    p = O.init_params(mc)
    for k in sorted(p):      # one generator per tensor: the SDF network's noise does not depend on the albedo network's shape
        t = p[k]
        gen = torch.Generator().manual_seed(1000 * seed + zlib.crc32(k.encode()))
        if k == "dev.variance":
            p[k] = torch.tensor(0.3 + 0.1 * float(torch.rand((), generator=gen)))
        elif k.endswith(".bias"):
            p[k] = t + 0.003 * torch.randn(t.shape, generator=gen)
        elif k.endswith(".weight_g"):
            p[k] = t * (1.0 + 0.02 * torch.randn(t.shape, generator=gen))
        else:
            rms = float(t.pow(2).mean().sqrt())
            p[k] = t + 0.03 * rms * torch.randn(t.shape, generator=gen)
    for name, w in pe_columns(p, mc).items():
        assert bool((w.abs().amax(dim=0) > 0).all()), f"{name}: a PE column is still zero"
    return p


def zero_blocks(p, mc, block=32):
    """(name, row block, column block) of every all-zero `block` x `block` tile of an effective weight, and every zero bias."""
    bad = []
    prefixes = [f"sdf.lin{l}" for l in range(mc.sdf.n_layers + 1)] + [f"color.lin{l}" for l in range(mc.color.n_layers + 1)]
    for pre in prefixes:
        w = _effective(p, pre)
        for r in range(0, w.shape[0], block):
            for c in range(0, w.shape[1], block):
                if not bool((w[r:r + block, c:c + block] != 0).any()):
                    bad.append((pre, r // block, c // block))
        if not bool((p[pre + ".bias"] != 0).all()):
            bad.append((pre + ".bias", -1, -1))
    return bad


def points(n, seed, lo=-0.9, hi=0.9):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, generator=g) * (hi - lo) + lo


def oracle_points(p, mc, pts, normals, feats, dt):
    """(sdf + feature [N, 1 + F], d sdf / dx [N, 3], albedo [N, d_out]) of the oracle in dtype dt."""
    q = {k: v.to(dt) for k, v in p.items()}
    x = pts.to(dt)
    with torch.no_grad():
        out = O.sdf_forward(q, mc.sdf, x)
        alb = O.color_forward(q, mc.color, x, normals.to(dt), normals.to(dt), feats.to(dt))
    nrm = O.sdf_gradient(q, mc.sdf, x, create_graph=False).detach()
    return out, nrm, alb


def step_batch(B=64):
    """the rays of every shape's end-to-end step"""
    return O.synthetic_batch(B, seed=11, step=1, warmup=False)


def desc_of(mc, **variant):
    """rnb_model_desc of `mc` as the drop-in classes write it (fields.model_desc), with the given variant bits."""
    import rnb_neus_fork_amd as R     # (the table itself needs no library)
    s, c = mc.sdf, mc.color
    sdf = R.SDFNetwork(d_in=3, d_out=s.d_out, d_hidden=s.d_hidden, n_layers=s.n_layers, skip_in=s.skip_in,
                       multires=s.multires, bias=s.bias, scale=s.scale, weight_norm=s.weight_norm)
    col = R.RenderingNetwork(d_feature=c.d_feature, mode=c.mode, d_in=c.d_in, d_out=c.d_out, d_hidden=c.d_hidden,
                             n_layers=c.n_layers, weight_norm=c.weight_norm, multires_view=c.multires_view,
                             squeeze_out=c.squeeze_out)
    d = R.model_desc(sdf, col)
    d.variant = R.native.variant_bits(**variant)
    return d
