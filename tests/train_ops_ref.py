"""fp64 references and input builders for the kernels that carry the parameters round a train step: the one-launch loss
(csrc/train.hip rnb_loss_kernel), the flat Adam (adam_kernel) and the weight-norm pair (csrc/weightnorm.hip).

A plain module (no device imports) shared by tests/test_train_ops_host.py (host: the references against the oracle and
torch, and every condition the device tests place on their inputs), tests/test_gpu_train_ops_edges.py and
tests/test_gpu_weightnorm.py.  Every reference takes a `dtype`: float64 is the yardstick, float32 is "what a plain fp32
implementation of the same formula gives", whose distance from fp64 calibrates the bounds (tests/parity.py)."""
from __future__ import annotations

import functools
import math
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle.bf16_emu import RS2, packed_layout
from tests.parity import rel_l2  # noqa: F401  (the tests take it as train_ops_ref.rel_l2)

# ----------------------------------------------------------------------------------------------------------------- loss
# The clip bounds of `weight_sum.clip(1e-3, 1.0 - 1e-3)` as an fp32 run sees them.  float32(1) - float32(1e-3) ==
# float32(0.999) = 0.99900001287..., above the double 0.999: an fp64 reference clipped at the double constants would
# disagree with every fp32 implementation about the sub-gradient at the boundary values.
CLIP_LO = float(np.float32(1e-3))
CLIP_HI = float(np.float32(1.0) - np.float32(1e-3))

# (B, L, color_depth): every B wraps or just misses the kernel's 1024-thread strided loops; L and color_depth make
# (i / Cd) % B wrong if it is wrong
LOSS_SHAPES = ((1, 1, 1), (63, 2, 3), (65, 5, 1), (1023, 1, 4), (1024, 2, 1), (1025, 5, 4), (4099, 1, 3), (1025, 2, 3))
LOSS_SHARDS = (37, 1, 90)           # a batch of 128 rays cut into three shards
IGR_W, MASK_W = 0.1, 0.1            # confs/wmask_rnb.conf:37-38

MASK_VALUES = (0.0, 0.25, 0.5, float(np.nextafter(np.float32(0.5), np.float32(1.0))), 0.75, 1.0)


def _f32(x):
    return np.float32(x)


def weight_sum_edges():
    """The 12 weight_sum values of the edge cases, fp32: outside, on and next to both clip bounds."""
    lo, hi = _f32(CLIP_LO), _f32(CLIP_HI)
    dn, up = _f32(-np.inf), _f32(np.inf)
    vals = [_f32(-0.5), _f32(0.0), _f32(1e-38), np.nextafter(lo, dn), lo, np.nextafter(lo, up), _f32(0.5),
            np.nextafter(hi, dn), hi, np.nextafter(hi, up), _f32(1.0), _f32(1.5)]
    return torch.tensor(np.array(vals, dtype=np.float32))


def _bce_terms(x, m):
    """binary_cross_entropy(reduction="none"); torch's own where it accepts the input (it refuses NaN), the same formula
    written out (both logs clamped at -100) otherwise."""
    if bool(torch.isfinite(x).all()):
        return F.binary_cross_entropy(x, m, reduction="none")
    return -(m * torch.log(x).clamp(min=-100.0) + (1.0 - m) * torch.log1p(-x).clamp(min=-100.0))


def loss_ref(color, rgb, mask, ws, ge, igr_w, mask_w, dtype, batch_global=None, eik_share=1.0):
    """oracle.rnb_oracle.rnb_loss in `dtype`, differentiable in color, ws and ge.  color, rgb: [L, B, Cd]; mask, ws: B
    values; ge: a scalar.  Returns (loss, {"color_loss", "eikonal_loss", "mask_loss"}).
    batch_global = (mask count, ray count) of a whole data-parallel batch: one shard's additive share (the sums over this
    shard's rays divided by the global counts, the eikonal term times eik_share)."""
    color, rgb, ws, ge = color.to(dtype), rgb.to(dtype), ws.to(dtype).reshape(-1, 1), ge.to(dtype)
    mask = mask.reshape(-1, 1)
    L = color.shape[0]
    m = (mask > 0.5).to(dtype) if mask_w > 0.0 else torch.ones(mask.shape, dtype=dtype)
    count = m.sum() if batch_global is None else torch.tensor(float(batch_global[0]), dtype=dtype)
    mask_sum = count + 1e-5
    err = ((color - rgb) * m[None, :, :]).reshape(-1, color.shape[-1])
    color_loss = F.l1_loss(err, torch.zeros_like(err), reduction="sum") / (mask_sum * L)
    x = ws.clip(CLIP_LO, CLIP_HI)
    if batch_global is None and bool(torch.isfinite(x).all()):
        mask_loss = F.binary_cross_entropy(x, m)              # the oracle's own call: fp32 runs agree bit for bit
    else:
        terms = _bce_terms(x, m)
        mask_loss = terms.mean() if batch_global is None else terms.sum() / float(batch_global[1])
    eik = ge if batch_global is None else ge * eik_share
    loss = color_loss + eik * igr_w + mask_loss * mask_w
    return loss, {"color_loss": color_loss, "eikonal_loss": eik, "mask_loss": mask_loss}


def loss_inputs(B, L, Cd, seed, mask_mode="mixed", special=None):
    """fp32 inputs of one loss case.  From ray 0 on, as far as B allows: the 12 weight_sum edges under mask 1, the same 12
    under mask 0, then one ray per mask value; a ray with color == rgb in every entry, a ray with -0.0 - (+0.0)
    differences, and single equal entries.  mask_mode: "mixed" (the six mask values), "zeros", "ones".
    special: "nan_ws" (ray B-1 has a NaN weight_sum), "inf_color" (one +inf colour entry on a masked-in ray B-2)."""
    g = torch.Generator().manual_seed(seed)
    color = torch.rand(L, B, Cd, generator=g)
    rgb = torch.rand(L, B, Cd, generator=g)
    ws = torch.rand(B, generator=g) * 1.2 - 0.1
    mv = torch.tensor(MASK_VALUES)
    mask = mv[torch.randint(0, len(mv), (B,), generator=g)]
    ge = torch.rand((), generator=g) + 0.05
    edges = weight_sum_edges()
    n = len(edges)
    for k, mval in enumerate((1.0, 0.0)):
        lo = k * n
        cnt = max(0, min(n, B - lo))
        ws[lo:lo + cnt] = edges[:cnt]
        mask[lo:lo + cnt] = mval
    lo = 2 * n
    cnt = max(0, min(len(mv), B - lo))
    mask[lo:lo + cnt] = mv[:cnt]
    if B > 40:
        color[:, 33] = rgb[:, 33]              # exact zeros of the L1 term on a whole ray, whatever its mask
        mask[34] = 1.0
        color[:, 34] = -0.0                    # -0.0 - (+0.0) = -0.0 on a masked-in ray
        rgb[:, 34] = 0.0
        mask[35] = 1.0
        color[0, 35, 0] = rgb[0, 35, 0]        # a single equal entry
    if mask_mode == "zeros":
        mask = torch.zeros(B)
    elif mask_mode == "ones":
        mask = torch.ones(B)
    if special == "nan_ws":
        ws[B - 1] = float("nan")
    elif special == "inf_color":
        mask[B - 2] = 1.0
        color[L - 1, B - 2, Cd - 1] = float("inf")
    return color, rgb, mask, ws, ge


def loss_ref_run(inp, igr_w, mask_w, dtype, upstream=1.0, batch_global=None, eik_share=1.0):
    """loss_ref and its three input gradients (of loss * upstream) on one input set: a dict of detached `dtype` tensors
    loss, color_loss, eikonal_loss, mask_loss, d_color [L, B, Cd], d_ws [B], d_ge []."""
    color, rgb, mask, ws, ge = inp
    leaves = [t.clone().to(dtype).requires_grad_(True) for t in (color, ws, ge)]
    loss, parts = loss_ref(leaves[0], rgb, mask, leaves[1], leaves[2], igr_w, mask_w, dtype, batch_global, eik_share)
    (loss * upstream).backward()
    out = {"loss": loss.detach()}
    out.update({k: v.detach() for k, v in parts.items()})
    out.update(d_color=leaves[0].grad, d_ws=leaves[1].grad, d_ge=leaves[2].grad)
    return out


# ----------------------------------------------------------------------------------------------------------------- Adam
ADAM_SETTINGS = {           # name: (betas, eps, weight_decay, steps of the long run)
    "default": ((0.9, 0.999), 1e-8, 0.0, 2000),
    "decay": ((0.9, 0.999), 1e-8, 1e-2, 2000),
    "fast_betas": ((0.5, 0.9), 1e-3, 0.0, 500),
    "tiny_eps": ((0.9, 0.999), 1e-15, 0.0, 500),
}
ADAM_SCALES = (1e-12, 1e-6, 1.0, 1e4)      # one parameter tensor per gradient scale; g^2 stays a normal fp32 number
ADAM_NUMEL = 1031
ADAM_ZERO_HEAD = 8                         # the first entries of every tensor get a gradient of exactly 0
ADAM_BASE_LR = 5e-4
ADAM_SEED = 11


def adam_lr(it, steps):
    """the schedule of tests/test_gpu_train_ops.py test_flat_adam_matches_torch_adam, stretched over `steps`"""
    return ADAM_BASE_LR * (0.5 + 0.5 * it / steps)


@functools.lru_cache(maxsize=None)
def adam_grad_sequence(steps=2000):
    """[steps, len(ADAM_SCALES), ADAM_NUMEL] fp32: the prescribed gradients (randn + 0.3) * scale, zero head per tensor.
    Shorter runs use a prefix of the 2,000-step sequence."""
    if steps != 2000:
        return adam_grad_sequence(2000)[:steps]
    g = torch.Generator().manual_seed(ADAM_SEED)
    seq = torch.randn(steps, len(ADAM_SCALES), ADAM_NUMEL, generator=g) + 0.3
    seq = seq * torch.tensor(ADAM_SCALES, dtype=torch.float32)[None, :, None]
    seq[:, :, :ADAM_ZERO_HEAD] = 0.0
    return seq


def adam_params0():
    g = torch.Generator().manual_seed(ADAM_SEED + 1)
    return torch.randn(len(ADAM_SCALES), ADAM_NUMEL, generator=g)


def _one_thread(fn):
    """thousands of steps on a few thousand elements: torch's intra-op thread pool costs a hundred times the arithmetic"""
    @functools.wraps(fn)
    def run(*a, **kw):
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            return fn(*a, **kw)
        finally:
            torch.set_num_threads(n)
    return run


@_one_thread
def adam_ref(p0, grads, lrs, betas, eps, wd, dtype):
    """The textbook Adam loop (torch.optim.Adam, amsgrad=False) in `dtype` on one flat tensor: grads and lrs are
    per-step sequences.  Returns (p, exp_avg, exp_avg_sq)."""
    b1, b2 = betas
    p = p0.detach().to(dtype).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for t, (g, lr) in enumerate(zip(grads, lrs), 1):
        g = g.to(dtype)
        if wd != 0.0:
            g = g + wd * p
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        denom = v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps
        p = p - (lr / (1.0 - b1 ** t)) * m / denom
    return p, m, v


@_one_thread
def torch_adam_run(p0, grads, lrs, betas, eps, wd, dtype, state_dict=None):
    """torch.optim.Adam on the CPU in `dtype` over one tensor per row of p0; returns (p, exp_avg, exp_avg_sq, optimizer)
    stacked like p0.  `state_dict`: loaded before the first step (a resumed run)."""
    ps = [torch.nn.Parameter(r.detach().to(dtype).clone()) for r in p0]
    opt = torch.optim.Adam(ps, lr=ADAM_BASE_LR, betas=betas, eps=eps, weight_decay=wd)
    if state_dict is not None:
        opt.load_state_dict(state_dict)
    for g, lr in zip(grads, lrs):
        for p, gi in zip(ps, g):
            p.grad = gi.to(dtype).clone()
        opt.param_groups[0]["lr"] = lr
        opt.step()
    st = opt.state_dict()["state"]
    stack = lambda key: torch.stack([st[i][key] for i in range(len(ps))])
    return torch.stack([p.detach() for p in ps]), stack("exp_avg"), stack("exp_avg_sq"), opt


@functools.lru_cache(maxsize=None)
def adam_long_refs(setting):
    """(fp64 textbook run, fp32 torch.optim.Adam run) of the long run of `setting`: two (p, m, v) triples shaped like
    adam_params0().  Computed once per setting and shared."""
    betas, eps, wd, steps = ADAM_SETTINGS[setting]
    seq = adam_grad_sequence(steps)
    lrs = [adam_lr(it, steps) for it in range(steps)]
    p0 = adam_params0()
    r64 = adam_ref(p0, seq, lrs, betas, eps, wd, torch.float64)
    r32 = torch_adam_run(p0, seq, lrs, betas, eps, wd, torch.float32)[:3]
    return r64, r32


def adam_moment_floor(beta):
    """The kernel forms 1.f - beta from the fp32 beta (2^-24 relative off the double 1 - beta, divided by 1 - beta): an
    EMA built on it differs from the ideal one by up to 2^-24 / (1 - beta), relative.  Four times that."""
    return 4.0 * 2.0 ** -24 / (1.0 - beta)


# ---------------------------------------------------------------------------------------------------------- weight norm
WN_SHAPES = ("default_64x64", "w100", "w32", "skip1", "nl1", "no_weight_norm", "mview0", "albedo_out4", "feat255")
WN_MISROUND_CAP = 1e-5              # share of real entries that may differ (by one ulp) from float32(fp64 product)


class Eff(NamedTuple):
    """One effective matrix with its places in the packed buffer.  W [N, K] in the reference's column order and b [N]:
    rows `rows` of the parameters `prefix`; w_slots [N, K], b_slots [N]: the float offset of each entry; wT_slots: of its
    transposed copy (None: the matrix has none)."""
    name: str
    prefix: str
    rows: slice
    W: torch.Tensor
    b: torch.Tensor
    w_slots: torch.Tensor
    b_slots: torch.Tensor
    wT_slots: Optional[torch.Tensor]


def _weight(q, prefix):
    """g * v / ||v|| per row (plain v without weight norm), as oracle/explicit.py eff_weights"""
    if prefix + ".weight" in q:
        return q[prefix + ".weight"]
    g, v = q[prefix + ".weight_g"], q[prefix + ".weight_v"]
    return v * (g / v.norm(dim=1, keepdim=True))


def _slots(e, N, K, col=None):
    r = torch.arange(N)[:, None]
    c = torch.arange(K)[None, :] if col is None else col[None, :]
    w = e["w"] + r * e["Kp"] + c
    wT = e["wT"] + c * e["Np"] + r if "wT" in e else None
    return w, e["b"] + torch.arange(N), wT


def wn_effective(p, mc, dtype):
    """The effective weights per layer, autograd kept (a `p` of `dtype` leaves that require grad gets their gradients):
    each row g v / ||v||, the skip layer times 1 / sqrt(2), and the map of every entry to its slot of the packed buffer
    (oracle.bf16_emu.packed_layout): hidden layers, the output layer as the sdf row (wsdf, bsdf) and the feature head,
    the albedo layers with layer 0's columns in the packed order [feature | pe(p) | pe(n)]."""
    L = packed_layout(mc)
    q = {k: v.to(dtype) for k, v in p.items()}
    sc, cc = mc.sdf, mc.color
    nh = sc.n_layers
    skip = sc.skip_in[0] if len(sc.skip_in) else -1
    out = []
    for l, e in enumerate(L["hid"]):
        pre = f"sdf.lin{l}"
        W = _weight(q, pre)
        if l == skip:
            W = W * RS2
        assert tuple(W.shape) == (e["N"], e["K"]), (pre, tuple(W.shape), e)
        out.append(Eff(pre, pre, slice(0, e["N"]), W, q[pre + ".bias"], *_slots(e, e["N"], e["K"])))
    pre = f"sdf.lin{nh}"
    W, b = _weight(q, pre), q[pre + ".bias"]
    H = sc.d_hidden
    out.append(Eff("sdf.head", pre, slice(0, 1), W[:1], b[:1], L["wsdf"] + torch.arange(H)[None, :],
                   torch.tensor([L["bsdf"]]), None))
    F_, pev = L["F"], L["pev"]
    if F_ > 0:
        out.append(Eff("sdf.feat", pre, slice(1, 1 + F_), W[1:], b[1:], *_slots(L["feat"], F_, H)))
        for l in range(cc.n_layers + 1):
            pre = f"color.lin{l}"
            e = L["col"][l] if l < cc.n_layers else L["colo"]
            col = None
            if l == 0:      # reference column i = [pe(p) | pe(n) | feature] -> packed column
                i = torch.arange(e["K"])
                col = torch.where(i < 2 * pev, F_ + i, i - 2 * pev)
            out.append(Eff(pre, pre, slice(0, e["N"]), _weight(q, pre), q[pre + ".bias"],
                           *_slots(e, e["N"], e["K"], col)))
    return out


def packed_regions(mc):
    """[(name, w offset, rows, columns, b offset or None, bias slots, wT offset or None)] of every block of the packed
    buffer, padding included, and the float offset where the last block ends."""
    L = packed_layout(mc)
    regs = []
    for l, e in enumerate(L["hid"]):
        regs.append((f"sdf.lin{l}", e["w"], e["Np"], e["Kp"], e["b"], e["Np"], e["wT"]))
    Hp = (mc.sdf.d_hidden + 31) // 32 * 32
    e = L["feat"]
    regs.append(("sdf.feat", e["w"], e["Np"], e["Kp"], e["b"], e["Np"], e["wT"]))
    regs.append(("sdf.head", L["wsdf"], 1, Hp, L["bsdf"], 1, None))
    for l, e in enumerate(L["col"]):
        regs.append((f"color.lin{l}", e["w"], e["Np"], e["Kp"], e["b"], e["Np"], e["wT"]))
    e = L["colo"]
    regs.append((f"color.lin{len(L['col'])}", e["w"], e["Np"], e["Kp"], e["b"], e["Np"], None))
    return regs, e["b"] + e["Np"]


def allowed_unwritten(mc):
    """The floats of [0, total) that rnb_weightnorm_fwd may leave alone: bsdf[1:32] (a 32-float slot of which the sdf
    bias uses the first) and the alignment tail behind the last block."""
    L = packed_layout(mc)
    ok = torch.zeros(L["total"], dtype=torch.bool)
    ok[L["bsdf"] + 1:L["bsdf"] + 32] = True
    ok[packed_regions(mc)[1]:] = True
    return ok


# the rows edited on one hidden layer and on albedo layer 0 (weight norm only)
ROW_G_ZERO, ROW_G_NEG, ROW_V_TINY, ROW_V_HUGE, ROW_V_ZERO = 1, 3, 4, 6, 7


def edited_layers(mc):
    """the hidden layer (lin1: the skip layer of the shape "skip1"; lin0 where there is one hidden layer) and albedo layer 0"""
    out = []
    if mc.sdf.weight_norm:
        out.append("sdf.lin1" if mc.sdf.n_layers > 1 else "sdf.lin0")
    if mc.color.weight_norm:
        out.append("color.lin0")
    return out


def wn_params(shape, zero_row):
    """live_params of `shape` with the row edits: g = 0, g < 0, v scaled by 1e-12 and by 1e+12, and (zero_row) a v row of
    zeros.  fp32, as the device receives them."""
    from tests.shape_matrix import live_params
    p = live_params(shape.mc, shape.seed)
    for pre in edited_layers(shape.mc):
        g, v = p[pre + ".weight_g"].clone(), p[pre + ".weight_v"].clone()
        assert g.shape[0] > ROW_V_ZERO
        g[ROW_G_ZERO] = 0.0
        g[ROW_G_NEG] = -g[ROW_G_NEG].abs() - 0.25
        v[ROW_V_TINY] = v[ROW_V_TINY] * 1e-12
        v[ROW_V_HUGE] = v[ROW_V_HUGE] * 1e12
        if zero_row:
            v[ROW_V_ZERO] = 0.0
        p[pre + ".weight_g"], p[pre + ".weight_v"] = g, v
    return p


def ulp_distance(a, b):
    """|a - b| in fp32 units in the last place (ordered-integer distance; +0 and -0 coincide); fp32 tensors, finite"""
    def ordered(x):
        i = x.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (ordered(a) - ordered(b)).abs()


def wn_objective(effs, c, dtype):
    """J = sum over the real slots of c[slot] * W_eff[slot] (weights and biases)"""
    J = 0.0
    for e in effs:
        J = J + (c[e.w_slots].to(dtype) * e.W).sum() + (c[e.b_slots].to(dtype) * e.b.reshape(-1)).sum()
    return J
