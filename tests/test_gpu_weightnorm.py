"""wn_fwd_kernel and wn_bwd_kernel (csrc/weightnorm.hip) called directly, element by element for every layer, against the
fp64 weight norm of tests/train_ops_ref.py (wn_effective: every matrix with its slots in the packed buffer).

Forward: into a NaN-filled buffer the test owns.  Every real entry is float32(fp64 product) up to one ulp, with at most
1e-5 of them not bit-equal (the kernel forms the row factor in fp64 and rounds each element once; its row sum differs from
torch's in summation order only); padding is +0.0, every W^T block the exact transpose, biases bit-equal, and the floats
left unwritten are bsdf[1:32] and the alignment tail.  Backward: a packed gradient that is NaN outside the real slots,
against torch autograd of J = sum c[slot] W_eff[slot] in fp64, calibrated by the same autograd in fp32.
tests/test_train_ops_host.py pins wn_effective, the slot map and the row edits.  Lines starting with WEIGHTNORM are
what profiles/train_ops_edges.txt is for."""
import ctypes as C
import functools

import pytest
import torch

from oracle.bf16_emu import packed_layout
from tests import train_ops_ref as T
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device
from tests.parity import check_value
from tests.shape_matrix import BY_NAME

pytestmark = pytest.mark.gpu

WN = [BY_NAME[n] for n in T.WN_SHAPES]
SENTINEL_BITS = 0x7FC0BEEF      # a quiet NaN with a payload no arithmetic produces: "this float was never written"


@functools.lru_cache(maxsize=None)
def _ref(name, zero_row):
    """(parameters, wn_effective in fp64) of one shape: computed once, shared by the tests"""
    shape = BY_NAME[name]
    p = T.wn_params(shape, zero_row)
    with torch.no_grad():
        effs = T.wn_effective(p, shape.mc, torch.float64)
    return p, effs


def _forward(R, shape, p, generic):
    """rnb_weightnorm_fwd of both networks into a sentinel-filled buffer; returns (fp32 buffer on the host, total)"""
    from rnb_neus_fork_amd.fields import _mlp_struct
    sdf, _, col, _ = R.build_from_named_params(shape.mc, p, device())
    desc = R.model_desc(sdf, col)
    desc.variant = R.native.variant_bits(generic=generic)
    n = R.runtime.packed_floats(desc)
    total = packed_layout(shape.mc)["total"]
    assert n == total if generic else n >= total
    packed = torch.full((n,), SENTINEL_BITS, dtype=torch.int32, device=device()).view(torch.float32)
    sp, cp = _mlp_struct(sdf.lins(), sdf.weight_norm), _mlp_struct(col.lins(), col.weight_norm)
    with R.native.on_device(packed) as stream:
        R.native.check(R.native.load().rnb_weightnorm_fwd(C.byref(desc), C.byref(sp), C.byref(cp), R.native.ptr(packed),
                                                          stream))
    torch.cuda.synchronize()
    return packed.cpu(), total


def _bits(x):
    return x.contiguous().view(torch.int32)


def _ranges(idx):
    """sorted indices -> "a..b" runs"""
    out, idx = [], idx.tolist()
    i = 0
    while i < len(idx):
        j = i
        while j + 1 < len(idx) and idx[j + 1] == idx[j] + 1:
            j += 1
        out.append(f"{idx[i]}..{idx[j]}")
        i = j + 1
    return out


@pytest.mark.parametrize("shape", WN, ids=lambda s: s.name)
def test_weightnorm_fwd_every_slot(R, shape):
    mc = shape.mc
    p, effs = _ref(shape.name, True)
    got, total = _forward(R, shape, p, generic=True)
    real = torch.zeros(total, dtype=torch.bool)
    n_real = n_differ = 0
    for e in effs:
        want = e.W.float()
        have = got[e.w_slots]
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(have), nan), f"{shape.name} {e.name}: NaN rows differ from the reference's"
        assert not bool((_bits(have) == SENTINEL_BITS).any()), f"{shape.name} {e.name}: a real entry was not written"
        d = T.ulp_distance(have[~nan], want[~nan])
        assert int(d.max()) <= 1, f"{shape.name} {e.name}: {int(d.max())} ulps from float32(fp64 product)"
        n_differ += int((d != 0).sum())
        n_real += int((~nan).sum())
        assert torch.equal(_bits(got[e.b_slots]), _bits(p[e.prefix + ".bias"][e.rows])), f"{shape.name} {e.name}: bias"
        real[e.w_slots.reshape(-1)] = True
        real[e.b_slots] = True
        if e.prefix in T.edited_layers(mc):
            assert bool((have[T.ROW_G_ZERO] == 0).all()), f"{e.name}: the g = 0 row is not zero"
            assert bool(torch.isnan(have[T.ROW_V_ZERO]).all()) and int(torch.isnan(have).any(dim=1).sum()) == 1
            neg = have[T.ROW_G_NEG].double() * p[e.prefix + ".weight_v"][T.ROW_G_NEG].double()
            assert bool((neg <= 0).all()) and bool((neg < 0).any()), f"{e.name}: the g < 0 row does not flip v"
    cap = T.WN_MISROUND_CAP * n_real
    print(f"WEIGHTNORM fwd {shape.name}: {n_differ} of {n_real} real entries not bit-equal to float32(fp64 product) (cap {cap:.1f})")
    assert n_differ <= cap
    # padding: every float of a W or bias block that is not a real entry is +0.0; every W^T block is the transpose
    regs, end = T.packed_regions(mc)
    block = torch.zeros(total, dtype=torch.bool)
    for name, w, n, k, b, nb, wT in regs:
        block[w:w + n * k] = True
        block[b:b + nb] = True
        if wT is not None:
            assert torch.equal(_bits(got[wT:wT + n * k]).view(k, n), _bits(got[w:w + n * k]).view(n, k).t()), \
                f"{shape.name} {name}: W^T is not the transpose of W"
    pad = block & ~real
    assert int(pad.sum()) > 0
    bad = (_bits(got[:total]) != 0) & pad
    assert not bool(bad.any()), f"{shape.name}: padding that is not +0.0 at floats {_ranges(bad.nonzero().flatten())[:8]}"
    # the floats nothing wrote
    unwritten = _bits(got[:total]) == SENTINEL_BITS
    print(f"WEIGHTNORM fwd {shape.name}: unwritten floats of [0, {total}): {_ranges(unwritten.nonzero().flatten())} "
          f"(bsdf[1:32] = {packed_layout(mc)['bsdf'] + 1}..{packed_layout(mc)['bsdf'] + 31}, tail from {end})")
    stray = unwritten & ~T.allowed_unwritten(mc)
    assert not bool(stray.any()), f"{shape.name}: unwritten floats outside bsdf[1:32] and the tail: {_ranges(stray.nonzero().flatten())[:8]}"


@pytest.mark.parametrize("shape", [s for s in WN if s.fused], ids=lambda s: s.name)
def test_weightnorm_fwd_default_variant_writes_the_same_fp32_part(R, shape):
    p, _ = _ref(shape.name, True)
    generic, total = _forward(R, shape, p, generic=True)
    default, _ = _forward(R, shape, p, generic=False)
    assert default.numel() > total, "a fused shape carries its mirrors behind the fp32 weights"
    assert torch.equal(_bits(default[:total]), _bits(generic)), f"{shape.name}: the fp32 part differs between the variants"


@pytest.mark.parametrize("shape", WN, ids=lambda s: s.name)
def test_weightnorm_bwd_every_leaf(R, shape):
    mc = shape.mc
    p, _ = _ref(shape.name, False)
    L = packed_layout(mc)
    total = L["total"]
    c = torch.randn(total, generator=torch.Generator().manual_seed(3))
    grads = {}
    for dt in (torch.float64, torch.float32):
        q = {k: v.clone().to(dt).requires_grad_(True) for k, v in p.items() if k != "dev.variance"}
        effs = T.wn_effective(q, mc, dt)
        T.wn_objective(effs, c, dt).backward()
        grads[dt] = {k: v.grad for k, v in q.items()}
    # the packed gradient as the renderer's backward hands it over (default variant: the mirrors lie behind `total`): c in
    # the real W and bias slots, NaN everywhere else
    sdf, _, col, _ = R.build_from_named_params(mc, p, device())
    desc = R.model_desc(sdf, col)
    n = R.runtime.packed_floats(desc)
    pgrad = torch.full((n,), float("nan"))
    b_slots = {}
    for e in effs:
        pgrad[e.w_slots] = c[e.w_slots]
        pgrad[e.b_slots] = c[e.b_slots]
        b_slots.setdefault(e.prefix, []).append(e.b_slots)
    assert bool(torch.isnan(pgrad[L["bsdf"] + 1:L["bsdf"] + 32]).all()) and int(torch.isfinite(pgrad).sum()) < total
    pgrad = pgrad.to(device())
    worst = ("", 0.0)
    for net, prefix, color in ((sdf, "sdf", False), (col, "color", True)):
        out = R.runtime._leaf_grads(desc, net, pgrad, color=color)
        torch.cuda.synchronize()
        names = [f"{prefix}.lin{l}.{leaf}" for l, lin in enumerate(net.lins())
                 for leaf in (("bias", "weight_g", "weight_v") if net.weight_norm else ("weight", "bias"))]
        assert len(names) == len(out)
        for name, g in zip(names, out):
            g = g.cpu()
            g64, g32 = grads[torch.float64][name], grads[torch.float32][name]
            assert g.shape == g64.shape
            assert bool(torch.isfinite(g).all()), f"{shape.name} {name}: a padded or mirrored gradient slot was read"
            pre = name.rsplit(".", 1)[0]
            if name.endswith(".bias"):
                assert torch.equal(g, c[torch.cat(b_slots[pre])]), f"{shape.name} {name}: not the packed slots bit for bit"
                continue
            rest = torch.ones(g.shape[0], dtype=torch.bool)
            if name.endswith(".weight_v") and pre in T.edited_layers(mc):
                assert bool((g[T.ROW_G_ZERO] == 0).all()), f"{name}: dv of the g = 0 row is not exactly 0"
                for row in (T.ROW_V_TINY, T.ROW_V_HUGE):     # dv scales inversely with v: relative to the row's own size
                    r = check_value(f"{shape.name} {name} row {row}", g[row], g64[row], g32[row],
                                    floor_scale=float(g64[row].abs().max()))
                    worst = max(worst, (f"{name}[{row}]", r), key=lambda t: t[1])
                    rest[row] = False
            r = check_value(f"{shape.name} {name}", g[rest], g64[rest], g32[rest])
            worst = max(worst, (name, r), key=lambda t: t[1])
    print(f"WEIGHTNORM bwd {shape.name}: worst error / bound {worst[1]:.3f} ({worst[0]})")
