"""One train step of RNB_VARIANT_BF16 against the bf16-emulating statement (oracle/bf16_emu.py), and the helpers it is
made of: shared by tests/test_gpu_bf16_emu.py (which states the bound rule), tests/test_gpu_shapes.py and
tests/test_gpu_ray_matrix.py.  Not a test module."""
import torch

from oracle import rnb_oracle as O
from oracle.bf16_emu import Bf16FinePass, packed_layout, weights_from_packed
from tests.golden_util import Golden
from tests.bf16_point_matrix import weighted_rnb_loss
from tests.gpu_support import device
from tests.parity import rel_l2

K = 4.0
FLOOR_RMS, FLOOR_LOSS, FLOOR_GRAD = 5e-5, 2e-5, 1e-4
# tests/test_gpu_bf16.py's bounds (SDF_ATOL, 3 SDF_ATOL for features, NRM_ATOL, OUT_ATOL, the loss's rel, GRAD_REL_MAX)
OLD = {"sdf": 1e-2, "feature": 3e-2, "normal": 1e-1, "out": 3e-2, "loss": 2e-2, "grad": 0.15}
OUT_KEYS = ("color_fine", "weights", "weight_sum", "cdf_fine", "gradients", "gradient_error")
MODES = ((torch.float32, "mm"), (torch.float32, "tiles"))


def model(R, mc, seed=0, sharpen=False, params=None, **variant):
    """`params`: the named parameters to build from (else the sharpened fixture's or a geometric init of `seed`)."""
    if params is not None:
        p = {k: v.clone() for k, v in params.items()}
    elif sharpen:
        p = Golden("full_main_sharp").params()
        with torch.no_grad():
            p["dev.variance"].fill_(0.3)     # inv_s = e^3, as in tests/test_gpu_bf16.py
    else:
        torch.manual_seed(seed)
        p = O.init_params(mc)
    sdf, dev, col, ren = R.build_from_named_params(mc, p, device())
    ren.set_variant(bf16=True, **variant)
    return p, sdf, dev, col, ren


def packed_weights(ren, mc):
    packed = ren._pack(True)
    total = packed_layout(mc)["total"]
    assert packed.numel() == total + total // 2, "RNB_VARIANT_BF16: fp32 weights + one bf16 mirror"
    return packed.cpu(), total


class Check:
    """Collects err(device), the emu32 errors and the bound of every quantity; prints all, then asserts all."""

    def __init__(self, tag):
        self.tag, self.rows = tag, []

    def add(self, name, e_dev, e32, floor, cap):
        bound = min(K * max(e32) + floor, cap)
        self.rows.append((name, e_dev, max(e32), bound))

    def output(self, name, dev, ref, others, old_bound):
        """A point-wise output: rms calibrated against emu32 (capped at old / 10), max-abs within old / 2."""
        dev, ref = dev.detach().cpu().double(), ref.detach().double()
        others = [o.detach().double() for o in others]
        rms = lambda a: float((a - ref).pow(2).mean().sqrt())
        self.add(name + " rms", rms(dev), [rms(o) for o in others], FLOOR_RMS, old_bound / 10)
        mx = lambda a: float((a - ref).abs().max())
        self.rows.append((name + " max", mx(dev), max(mx(o) for o in others), old_bound / 2))

    def worst(self):
        """the largest device / emu32 ratio over the calibrated rows (rms, loss, gradients) and the largest share of a bound"""
        cal = [(e / max(e32, 1e-30), n) for n, e, e32, _ in self.rows if not n.endswith(" max")]
        return {"worst_ratio": max(cal), "worst_of_bound": max((e / b, n) for n, e, _, b in self.rows)}

    def finish(self):
        for name, e, e32, bound in self.rows:
            print(f"BF16EMU {self.tag} {name}: device {e:.3e}, emu32 {e32:.3e}, ratio {e / max(e32, 1e-30):.2f}, "
                  f"bound {bound:.3e}")
        bad = [f"{n}: {e:.3e} > {b:.3e}" for n, e, _, b in self.rows if not e <= b]
        assert not bad, f"{self.tag}: " + "; ".join(bad)


def step_loss(api, out, b, rw=None):
    """`rw` [B]: per-ray weights of the colour and mask terms (tests/bf16_point_matrix.py weighted_rnb_loss; render_rnb only)"""
    if rw is not None:
        assert api == "render_rnb"
        return weighted_rnb_loss(out, b["true_rgb"], b["mask"], rw)
    if api == "render":
        return (out["color_fine"] - b["true_rgb"][0]).abs().mean() + 0.1 * out["gradient_error"] \
            + 0.1 * torch.nn.functional.binary_cross_entropy(out["weight_sum"].clip(1e-3, 1 - 1e-3),
                                                             (b["mask"] > 0.5).to(out["weight_sum"].dtype))
    return O.rnb_loss(out, b["true_rgb"], b["mask"])[0]


def emulated_step(p, mc, w, batch, z, api, no_albedo, bg, dt, order, rw=None):
    fp = Bf16FinePass(p, mc, w, dtype=dt, order=order)
    warm = api == "render_rnb_warmup"
    if api == "render":
        out = fp.forward(batch["rays_o"], batch["rays_d"], z, None, cos_anneal_ratio=1.0, relu_shading=False,
                         no_albedo=False, mvps=False, background_rgb=bg)
    else:
        out = fp.forward(batch["rays_o"], batch["rays_d"], z, batch["lights_dir"], cos_anneal_ratio=1.0,
                         relu_shading=warm, no_albedo=no_albedo, mvps=True)
    leaves = {k: out[k].detach().clone().requires_grad_(True) for k in ("color_fine", "weight_sum", "gradient_error")}
    bt = {k: v.to(dt) for k, v in batch.items()}
    loss = step_loss(api, {**out, **leaves}, bt, rw)
    loss.backward()
    grads = fp.backward({k: v.grad for k, v in leaves.items()})
    return out, float(loss), grads


def tail_ray_weight(p, mc, w, batch, z, api, no_albedo, key):
    """the weight of the LAST ray at which, in the fp64 emulation, it carries half of the norm of `key`'s gradient: two
    backward passes, with the last ray alone and with the rest alone (the loss is linear in the ray weights)"""
    B = z.shape[0]
    last = torch.zeros(B, dtype=torch.float64)
    last[B - 1] = 1.0
    g_last = emulated_step(p, mc, w, batch, z, api, no_albedo, None, torch.float64, "mm", rw=last)[2][key]
    g_rest = emulated_step(p, mc, w, batch, z, api, no_albedo, None, torch.float64, "mm", rw=1.0 - last)[2][key]
    n_last, n_rest = float(g_last.norm()), float(g_rest.norm())
    assert n_last > 0 and n_rest > 0, f"the last ray or the rest carries no gradient of {key}"
    rw = torch.ones(B, dtype=torch.float64)
    rw[B - 1] = n_rest / n_last
    return rw


def step(R, mc, B, api="render_rnb", no_albedo=False, sharpen=True, seed=2, tag="", params=None, batch=None, z_vals=None,
         tail_key=None, info=None, **variant):
    """`batch`: the rays (else the synthetic batch of B); `z_vals` [B, S]: explicit depths instead of sampling; `tail_key`
    (with z_vals): the last ray's loss weight is set by tail_ray_weight on that gradient; `info`: a dict that receives the
    worst device / emu32 ratios and the ray weight."""
    p, sdf, dev, col, ren = model(R, mc, seed=seed, sharpen=sharpen, params=params, **variant)
    warm = api == "render_rnb_warmup"
    if batch is None:
        batch = O.synthetic_batch(B, seed=40 + B, step=1, warmup=warm)
    b = {k: v.to(device()) for k, v in batch.items()}
    depths = dict(t_rand=b["t_rand"]) if z_vals is None else dict(z_vals=z_vals.to(device()))
    rw = None
    if tail_key is not None:
        packed, total = packed_weights(ren, mc)
        rw = tail_ray_weight(p, mc, weights_from_packed(packed[:total], mc), batch, z_vals, api, no_albedo, tail_key)
    bg = None
    if api == "render":
        bg = torch.tensor([0.2, 0.5, 0.8])
        out = ren.render(b["rays_o"], b["rays_d"], b["near"], b["far"], background_rgb=bg.to(device()), cos_anneal_ratio=1.0,
                         **depths)
    else:
        fn = ren.render_rnb_warmup if warm else ren.render_rnb
        out = fn(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=1.0, no_albedo=no_albedo,
                 **depths)
    loss = step_loss(api, out, b, rw)
    loss.backward()
    torch.cuda.synchronize()
    z = ren.last_z_vals.cpu()
    packed, total = packed_weights(ren, mc)
    w = weights_from_packed(packed[:total], mc)
    emu = [emulated_step(p, mc, w, batch, z, api, no_albedo, bg, dt, order, rw)
           for dt, order in ((torch.float64, "mm"),) + MODES]
    (o64, l64, g64), rest = emu[0], emu[1:]
    chk = Check(tag or f"{api} B={B} S={z.shape[1]} no_albedo={no_albedo} {variant}")
    for k in OUT_KEYS:
        assert bool(torch.isfinite(out[k]).all()), k
        chk.output(k, out[k], o64[k], [o[k] for o, _, _ in rest], OLD["normal"] if k == "gradients" else OLD["out"])
    chk.add("loss", abs(float(loss) - l64) / abs(l64), [abs(l - l64) / abs(l64) for _, l, _ in rest], FLOOR_LOSS,
            OLD["loss"] / 10)
    named = {("sdf." + k): v for k, v in sdf.named_parameters()}
    named["dev.variance"] = dev.variance
    named.update({("color." + k): v for k, v in col.named_parameters()})
    n_checked = 0
    for k, v in named.items():
        if k not in g64:
            assert v.grad is None or float(v.grad.abs().max()) == 0.0, f"{k}: a gradient the emulation does not have"
            continue
        assert v.grad is not None, f"{k}: no device gradient"
        ref = g64[k].reshape(v.shape).detach()
        if float(ref.norm()) == 0.0:
            assert float(v.grad.abs().max()) == 0.0, k
            continue
        chk.add(k, rel_l2(v.grad.detach().cpu(), ref), [rel_l2(g[k].reshape(v.shape).detach(), ref) for _, _, g in rest],
                FLOOR_GRAD, OLD["grad"] / 10)
        n_checked += 1
    if info is not None:
        info.update(chk.worst(), ray_weight=None if rw is None else float(rw[-1]))
    chk.finish()
    return n_checked


def linspace_at(lo, hi, res, i):
    """rnb_internal.h linspace_at in exact fp32: step = fp32((hi - lo) / (res - 1)), then one fused multiply-add."""
    lo32, hi32 = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    step = (hi32 - lo32) / torch.tensor(float(res - 1), dtype=torch.float32)
    i = torch.as_tensor(i, dtype=torch.float64)
    a = step.double() * i + lo32.double()
    b = -step.double() * (res - 1 - i) + hi32.double()
    return torch.where(i < res // 2, a, b).float()
