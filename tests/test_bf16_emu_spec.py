"""The bf16-emulating statement (oracle/bf16_emu.py) that tests/test_gpu_bf16_emu.py holds the bf16 variant to.  CPU only.

  - with every rounding site off it IS the explicit statement (oracle/explicit.py) in fp64: outputs and gradients ~1e-12;
  - every rounding site is wired to something: switching one off changes an output or a gradient;
  - `rb` is round-to-nearest-even with the kernel conversion's edge behaviour (v_cvt_pk_bf16_f32);
  - with every site on, emu64 is about bf16's error away from unrounded fp64: above 1e-4, below tests/test_gpu_bf16.py's
    bounds (an emulation that rounds nothing or rounds twice fails here)."""
import pytest
import torch

from oracle import rnb_oracle as O
from oracle.bf16_emu import SITES, Bf16FinePass, rb, weights_from_params
from oracle.explicit import FinePass
from tests.golden_util import Golden
from tests.parity import rel_l2

OUT_KEYS = ["color_fine", "weights", "weight_sum", "weight_max", "gradients", "gradient_error", "cdf_fine", "s_val"]


def _to64(d):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}


def _case(name, n_rays=None):
    g = Golden(name)
    p = _to64(g.params())
    b = _to64(g.batch)
    z = g.steps[-1]["z_out"].double()
    if n_rays is not None:
        b = {k: (v[:, :n_rays] if k in ("true_rgb", "lights_dir") else v[:n_rays]) if torch.is_tensor(v) and v.dim() > 0
             else v for k, v in b.items()}
        z = z[:n_rays]
    kw = dict(cos_anneal_ratio=g.cos_anneal_ratio)
    if g.api == "render":
        kw.update(relu_shading=False, no_albedo=False, mvps=False, background_rgb=b.get("background_rgb"))
        lights = None
    else:
        kw.update(relu_shading=(g.api == "render_rnb_warmup"), no_albedo=g.no_albedo, mvps=True)
        lights = b["lights_dir"]
    return g, p, b, z, lights, kw


def _run(fp, b, z, lights, kw, cot=None):
    out = fp.forward(b["rays_o"], b["rays_d"], z, lights, **kw)
    if cot is None:
        gen = torch.Generator().manual_seed(5)
        cot = {k: torch.randn(out[k].shape, generator=gen, dtype=torch.float64) for k in OUT_KEYS}
    return out, fp.backward(cot), cot


@pytest.mark.parametrize("name", ["tiny_main_sharp", "tiny_warmup_sharp", "tiny_main_noalbedo", "tiny_render_bg",
                                  "full_main_sharp"])
def test_unrounded_emulation_is_the_explicit_statement(name):
    g, p, b, z, lights, kw = _case(name, n_rays=8 if name.startswith("full") else None)
    ref = FinePass(p, g.mc)
    out_r, gr_r, cot = _run(ref, b, z, lights, kw)
    for color_bf16 in (False, True):
        emu = Bf16FinePass(p, g.mc, weights_from_params(p, g.mc), sites=(), color_bf16=color_bf16)
        out_e, gr_e, _ = _run(emu, b, z, lights, kw, cot)
        for k in OUT_KEYS:
            torch.testing.assert_close(out_e[k], out_r[k], rtol=1e-11, atol=1e-12, msg=lambda m: f"{k}: {m}")
        assert set(gr_e) == set(gr_r)
        for k, v in gr_r.items():
            if float(v.norm()) == 0.0:
                assert float(gr_e[k].norm()) == 0.0, k
                continue
            assert rel_l2(gr_e[k], v) < 1e-10, f"{k}: {rel_l2(gr_e[k], v):.2e}"


def test_every_rounding_site_is_live():
    """Each site, switched off alone, changes at least one output or gradient (tiny network, the albedo net in bf16 so
    that its sites are reached)."""
    g, p, b, z, lights, kw = _case("tiny_main_sharp")
    w = weights_from_params(p, g.mc)
    full_out, full_gr, cot = _run(Bf16FinePass(p, g.mc, w, color_bf16=True), b, z, lights, kw)
    for s in SITES:
        out, gr, _ = _run(Bf16FinePass(p, g.mc, w, sites=set(SITES) - {s}, color_bf16=True), b, z, lights, kw, cot)
        d = max([float((out[k] - full_out[k]).abs().max()) for k in OUT_KEYS]
                + [float((gr[k] - full_gr[k]).abs().max()) for k in full_gr])
        assert d > 0.0, f"rounding site {s!r} changes nothing"
    # ... and the fp32 albedo path does not round the albedo sites
    out0, gr0, _ = _run(Bf16FinePass(p, g.mc, w, color_bf16=False), b, z, lights, kw, cot)
    out1, gr1, _ = _run(Bf16FinePass(p, g.mc, w, sites=set(SITES) - {"feat", "cpe", "cact", "zc"}, color_bf16=False),
                        b, z, lights, kw, cot)
    for k in OUT_KEYS:
        assert torch.equal(out0[k], out1[k]), k
    for k in gr0:
        assert torch.equal(gr0[k], gr1[k]), k


def _bits(x):
    return int(torch.tensor([x], dtype=torch.float32).view(torch.int32)[0]) & 0xFFFFFFFF


def _f32(bits):
    return torch.tensor([bits if bits < 2 ** 31 else bits - 2 ** 32], dtype=torch.int32).view(torch.float32)


def _rb_bits(bits):
    y = rb(_f32(bits))
    assert y.dtype == torch.float32
    return _bits(float(y[0])) if not torch.isnan(y).any() else None


def test_rb_rounds_to_nearest_even():
    # 1 + half a bf16 ulp (2^-8) is a tie: the even neighbour is 1.0; 1 + 3/2 ulp goes up to 1 + 2 ulp
    assert _rb_bits(0x3F808000) == 0x3F800000
    assert _rb_bits(0x3F818000) == 0x3F820000
    assert _rb_bits(0xBF808000) == 0xBF800000         # the sign does not matter
    # one fp32 ulp above the tie rounds up, one below rounds down
    assert _rb_bits(0x3F808001) == 0x3F810000
    assert _rb_bits(0x3F807FFF) == 0x3F800000
    # exact bf16 values pass unchanged
    for v in (0.0, -0.0, 1.0, -2.5, 0.0078125, 3.0e38):
        t = torch.tensor([v], dtype=torch.float32)
        if _bits(v) & 0xFFFF == 0:
            assert torch.equal(rb(t), t)


def test_rb_subnormals_inf_nan_overflow():
    # subnormals keep their bits and round like normal numbers (v_cvt_pk_bf16_f32 does not flush them)
    assert _rb_bits(0x00008000) == 0x00000000         # tie below the smallest bf16 subnormal: to even (zero)
    assert _rb_bits(0x00018000) == 0x00020000         # tie: up to the even neighbour
    assert _rb_bits(0x00010001) == 0x00010000
    assert _rb_bits(0x00010000) == 0x00010000         # the smallest bf16 subnormal itself
    assert _rb_bits(0x007FFFFF) == 0x00800000         # the largest fp32 subnormal rounds up to the smallest normal
    # infinities pass through, NaN stays NaN
    assert _rb_bits(0x7F800000) == 0x7F800000
    assert _rb_bits(0xFF800000) == 0xFF800000
    assert _rb_bits(0x7FC00000) is None and _rb_bits(0x7F800001) is None
    # the bf16 maximum is 0x7F7F; half an ulp above it (a tie with an odd mantissa) and beyond overflow to inf
    assert _rb_bits(0x7F7F0000) == 0x7F7F0000
    assert _rb_bits(0x7F7F7FFF) == 0x7F7F0000
    assert _rb_bits(0x7F7F8000) == 0x7F800000
    assert _rb_bits(0x7F7FFFFF) == 0x7F800000
    assert _rb_bits(0xFF7F8000) == 0xFF800000
    # float64 operands round through fp32, as the device rounds an fp32 value: 1 + 2^-8 + 2^-40 is first the fp32 tie
    # 1 + 2^-8, then 1.0 (emu64 thus rounds what an exact fp32 epilogue would have produced)
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert float(rb(x)[0]) == 1.0


def test_emu64_is_about_bf16_error_from_fp64():
    """Full-size network: the rounded statement is away from the unrounded one by bf16's error (well above fp32's),
    and within the coarse bounds of tests/test_gpu_bf16.py."""
    torch.set_num_threads(16)
    g, p, b, z, lights, kw = _case("full_main_sharp", n_rays=16)
    p["dev.variance"].fill_(0.3)         # tests/test_gpu_bf16.py's sharpened model: inv_s = e^3
    w = weights_from_params(p, g.mc)
    ref_out, ref_gr, cot = _run(Bf16FinePass(p, g.mc, w, sites=()), b, z, lights, kw)
    out, gr, _ = _run(Bf16FinePass(p, g.mc, w), b, z, lights, kw, cot)
    e_n = float((out["gradients"] - ref_out["gradients"]).abs().max())
    e_w = max(float((out[k] - ref_out[k]).abs().max()) for k in ("color_fine", "weights", "weight_sum", "cdf_fine"))
    print(f"emu64 vs unrounded fp64: normals {e_n:.2e}, render outputs {e_w:.2e}")
    assert 1e-4 < e_n <= 1e-1
    assert 1e-4 < e_w <= 3e-2
    rels = {k: rel_l2(gr[k], ref_gr[k]) for k in ref_gr if float(ref_gr[k].norm()) > 0}
    worst = max(rels, key=rels.get)
    print(f"emu64 vs unrounded fp64: gradient rel-L2 median {sorted(rels.values())[len(rels) // 2]:.2e}, "
          f"worst {worst} {rels[worst]:.2e}")
    assert max(rels.values()) <= 0.15
    assert sorted(rels.values())[len(rels) // 2] > 1e-4
