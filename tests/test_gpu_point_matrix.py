"""The point-tiled kernels of the shipped 256-wide route over the table of tests/point_matrix.py, on the device.

Every row (a point count M) runs through the direct network calls with set_autograd(True), on default_64x64 in the default
arithmetic, once per backward kind of the table (feature, eikonal, color, texture), against the torch oracle in fp64 with the
fp32 oracle calibrating (tests/parity.py check_value / check_grad, unchanged; the helpers of tests/field_autograd_util.py).
Per row and kind:
  1. the outputs (sdf, feature, normal, albedo), every leaf gradient (the bias gradients among them, one by one: they are
     the column sums behind gemm_dw_x3_kernel's `c + 2 < nchunks` guard) and every input gradient;
  2. the last min(M, 64) rows of every per-point input gradient as a tensor of their own;
  3. the same again with the adjoint weights of the last rows scaled so that, in the fp64 oracle, those rows carry half of the
     norm of lin1.weight_v's gradient: a 16-point chunk that is dropped, doubled or read from padding then moves a gradient at
     order one at every M (with plain weights it moves it by ~16 / M).  "The last rows" are the last min(32, M // 2): 32, or
     at M = 32 and 33 the last 16, the one chunk that the kernel's second register set holds;
  4. the route, from the library's profiler: the sweeps of the kind; for M % 32 == 0 the one-workgroup weight-gradient
     kernel and its slab reduction and no split-K launch, otherwise the split-K kernels alone.  This is the one place where
     the plan restated in tests/point_matrix.py meets the library on the device.
A leaf whose fp64 gradient vanishes must be exactly zero on the device; a leaf the fp32 oracle resolves to worse than
GRAD_CAP / K_GRAD is refused as a parity target (none is skipped).  Every case prints one POINTROW line.

Then: four rows with x2h=False (six bf16 terms, NP = 3: another LDS image of the same pipeline), the ragged rows with
deterministic=True (twice, bit for bit), and three render steps whose ray count x samples puts the composite and the loss
in front of the same tails."""
from dataclasses import replace

import pytest
import torch

from oracle import rnb_oracle as O
from tests import parity as P
from tests import point_matrix as PM
from tests import ray_matrix as RM
from tests.field_autograd_util import build, check_grad_or_zero, compare_leaves, mesh_texture, native_leaf_grads, oracle, \
    oracle_normal, weights, zero_grads
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import ALBEDO_H2_CLASSES, FUSED_CLASSES, device, profile_classes, step_against_fp64
from tests.shape_matrix import BY_NAME as SHAPE_BY_NAME, live_params, points

pytestmark = pytest.mark.gpu

SHAPE = "default_64x64"
X3, REDUCE, SPLIT_K = "dW(x3: 256x256 + narrow jobs)", "dW(slab reduce)", "dW(other)"
SDF_SWEEPS = {"feature": {"F_sweep(save)", "FB_sweep"}, "eikonal": {"F_sweep(save)", "R_sweep", "RA_sweep", "FB_sweep"}}
SWEEPS = dict(SDF_SWEEPS, color=set(ALBEDO_H2_CLASSES),
              texture=SDF_SWEEPS["feature"] | SDF_SWEEPS["eikonal"] | set(ALBEDO_H2_CLASSES))
TAIL_SLICE = 64


def tail_rows(M):
    return min(32, M // 2)


@pytest.fixture(scope="module")
def nets(R):
    return build(R, SHAPE)


class Case:
    """inputs, oracle loss and native call of one (M, kind); `rw` [M, 1]: the adjoint weight of every row"""

    def __init__(self, mc, M, kind):
        self.M, self.kind, self.sc, self.cc = M, kind, mc.sdf, mc.color
        F = self.sc.d_out - 1
        if kind == "color":
            self.inputs = [points(M, seed=M + 7), torch.nn.functional.normalize(weights(M, 3, 3), dim=-1),
                           0.5 * weights(M, self.cc.d_feature, 4)]
            self.input_names = ("points", "normals", "feats")
        else:
            self.inputs = [points(M, seed=M + {"feature": 0, "eikonal": 5, "texture": 11}[kind])]
            self.input_names = ("x",)
        self.W1, self.WF, self.Wc = weights(M, 1, 1), weights(M, F, 2), weights(M, self.cc.d_out, 5)
        self.prefix = {"feature": "sdf.", "eikonal": "sdf.", "color": "color.", "texture": ""}[kind]
        self.key = ("color" if kind == "color" else "sdf") + ".lin1.weight_v"      # the leaf the tail factor is chosen on
        self.out_names = {"feature": ("sdf", "feature"), "eikonal": ("normal",), "color": ("albedo",), "texture": ("albedo",)}[kind]

    def _loss(self, outs, rw):
        if self.kind == "feature":
            o = outs[0]
            return (rw.to(o) * self.W1.to(o) * o[:, :1]).sum() + (rw.to(o) * self.WF.to(o) * o[:, 1:]).sum()
        if self.kind == "eikonal":
            g = outs[0]
            return (rw.to(g)[:, 0] * (g.norm(dim=-1) - 1) ** 2).sum() / self.M
        a = outs[0]
        return (rw.to(a) * self.Wc.to(a) * a).sum()

    def oracle_fn(self, rw):
        def fn(q, *xs):
            if self.kind == "feature":
                out = O.sdf_forward(q, self.sc, xs[0])
            elif self.kind == "eikonal":
                out = oracle_normal(q, self.sc, xs[0])
            elif self.kind == "color":
                out = O.color_forward(q, self.cc, xs[0], xs[1], xs[1], xs[2])
            else:
                nrm = oracle_normal(q, self.sc, xs[0])
                out = O.color_forward(q, self.cc, xs[0], nrm, nrm, O.sdf_forward(q, self.sc, xs[0])[:, 1:])
            return out, self._loss([out], rw)
        return fn

    def oracle(self, p, rw, dt, dev=None):
        out, g, ins = oracle(p, self.prefix, self.inputs, self.oracle_fn(rw), dt, dev)
        return out, {k: v for k, v in g.items() if k.startswith(("sdf.", "color."))}, ins

    def split_outputs(self, out):
        return (out[:, :1], out[:, 1:]) if self.kind == "feature" else (out,)

    def native(self, sdf, col, rw):
        """(output, {leaf: grad}, [input grads]) of the device"""
        zero_grads(sdf, col)
        xs = [t.to(device()).requires_grad_(True) for t in self.inputs]
        if self.kind == "feature":
            out = sdf(xs[0])
        elif self.kind == "eikonal":
            out = sdf.gradient(xs[0]).reshape(self.M, 3)
        elif self.kind == "color":
            out = col(xs[0], xs[1], xs[1].detach(), xs[2])
        else:
            out = mesh_texture(sdf, col, xs[0])
        assert out.grad_fn is not None
        self._loss([out], rw.to(device())).backward()
        mine = {}
        if self.kind != "color":
            mine.update(native_leaf_grads(sdf, "sdf"))
        if self.kind in ("color", "texture"):
            mine.update(native_leaf_grads(col, "color"))
        for t, name in zip(xs, self.input_names):
            assert t.grad is not None, f"{name}.grad: none"
        return out.detach(), {k: v.clone() for k, v in mine.items()}, [t.grad.clone() for t in xs]

    def tail_weights(self, p):
        """row weights 1 (head) and s (the last tail_rows(M) rows), s chosen on the fp64 oracle so that the tail's share of
        d loss / d lin1.weight_v has the norm of the head's; the loss is linear in the row weights"""
        M, t = self.M, tail_rows(self.M)
        ones = torch.ones(M, 1)
        only = torch.zeros(M, 1)
        only[M - t:] = 1.0
        g_all = self.oracle(p, ones, torch.float64)[1][self.key]
        g_tail = self.oracle(p, only, torch.float64)[1][self.key]
        n_head, n_tail = float((g_all - g_tail).norm()), float(g_tail.norm())
        assert n_tail > 0 and n_head > 0, f"M={M} {self.kind}: the head or the tail carries no gradient of {self.key}"
        s = n_head / n_tail
        rw = ones.clone()
        rw[M - t:] = s
        return rw, s


def check_case(case, p, sdf, col, rw, tag, stats):
    """one pass of a case with row weights rw against the fp64 oracle; the worst ratios go to stats"""
    o64, g64, i64 = case.oracle(p, rw, torch.float64)
    o32, g32, i32 = case.oracle(p, rw, torch.float32)
    out, mine, ins = case.native(sdf, col, rw)
    torch.cuda.synchronize()

    def note(group, name, ratio):
        if ratio >= stats.get(group, ("", -1.0))[1]:
            stats[group] = (name, ratio)
    for name, got, r64, r32 in zip(case.out_names, case.split_outputs(out), case.split_outputs(o64), case.split_outputs(o32)):
        note("out", name, P.check_value(f"{tag} {name}", got, r64.cpu(), r32.cpu()))
    for k in g64:       # (the rule of step_against_fp64: a leaf the fp32 oracle does not resolve is not a parity target)
        if float(g64[k].abs().max()) > 0.0:
            rel32 = P.rel_l2(g32[k], g64[k])
            assert rel32 <= P.GRAD_CAP / P.K_GRAD, f"{tag} {k}: the fp32 oracle itself is {rel32:.2e} from fp64: not a parity target"
    for k, ratio in compare_leaves(mine, g64, g32, tag).items():
        note("bias" if k.endswith(".bias") else "grad", k, ratio)
    n_tail = min(case.M, TAIL_SLICE)
    for name, got, r64, r32 in zip(case.input_names, ins, i64, i32):
        note("grad", f"{name}.grad", check_grad_or_zero(got, r64, r32, f"{tag} {name}.grad"))
        note("tail", f"{name}.grad[-{n_tail}:]",
             check_grad_or_zero(got[-n_tail:], r64[-n_tail:], r32[-n_tail:], f"{tag} {name}.grad, the last {n_tail} rows"))
    return mine, ins


def assert_dw_route(M, classes, tag):
    if PM.runs_x3(M):
        assert {X3, REDUCE} <= classes and SPLIT_K not in classes, f"{tag}: M % 32 == 0 must take the one-workgroup kernel: {sorted(classes)}"
    else:
        assert X3 not in classes and SPLIT_K in classes, f"{tag}: M % 32 != 0 must take the split-K kernels: {sorted(classes)}"


def run_row(R, nets, M, kind, tag, sweeps=True):
    """both passes of a (row, kind) with the route assertion and the POINTROW line; returns the gradients of the first pass"""
    shape, p, sdf, col, ren = nets
    lib = R.native.load()
    case = Case(shape.mc, M, kind)
    stats = {}
    lib.rnb_profile_enable(1)
    try:
        first = check_case(case, p, sdf, col, torch.ones(M, 1), f"{tag} M={M} {kind}", stats)
        classes = profile_classes(R)
    finally:
        lib.rnb_profile_enable(0)
    assert_dw_route(M, classes, f"{tag} M={M} {kind}")
    if sweeps:
        assert SWEEPS[kind] <= classes, f"{tag} M={M} {kind}: sweeps missing: {sorted(SWEEPS[kind] - classes)}"
        if kind == "feature":
            assert "RA_sweep" not in classes, "a backward without the normal runs no RA sweep"
    rw, s = case.tail_weights(p)
    tstats = {}
    check_case(case, p, sdf, col, rw, f"{tag} M={M} {kind} tail x{s:.3g}", tstats)
    f = lambda st, g: f"{st[g][0]} {st[g][1]:.2f}"
    print(f"POINTROW {tag} M={M} Mp={PM.pad_rows(M)} fwd {PM.forward_family(M)} {kind}: classes {sorted(classes)}; worst output "
          f"{f(stats, 'out')}, gradient {f(stats, 'grad')}, bias {f(stats, 'bias')}, tail slice {f(stats, 'tail')} of its bound; "
          f"tail-heavy (last {tail_rows(M)} rows x {s:.3g}): output {f(tstats, 'out')}, gradient {f(tstats, 'grad')}, bias "
          f"{f(tstats, 'bias')}, tail slice {f(tstats, 'tail')}")
    return first


# ------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("kind", PM.KIND_NAMES)
@pytest.mark.parametrize("row", PM.ROWS, ids=[repr(r) for r in PM.ROWS])
def test_point_row_against_fp64(R, nets, row, kind):
    run_row(R, nets, row.M, kind, "default")


# ------------------------------------------------------------------------------------------------------------------- 2
def _set_variant(monkeypatch, R, **variant):
    """the direct calls build their own descriptors (runtime.model_desc / _color_desc): the variant bits go in there, as
    tests/test_gpu_operand_range.py test_variant_switch_reaches_the_point_entry_points puts them into its own"""
    bits = R.native.variant_bits(**variant)
    for name in ("model_desc", "_color_desc"):
        plain = getattr(R.runtime, name)

        def with_bits(*a, _plain=plain, **k):
            d = _plain(*a, **k)
            d.variant = bits
            return d
        monkeypatch.setattr(R.runtime, name, with_bits)


@pytest.mark.parametrize("M", PM.SHORT_ROWS)
def test_six_term_arithmetic_on_the_short_rows(R, nets, monkeypatch, M):
    """x2h=False: dw_x3_body with NP = 3 (three planes per operand: another LDS image and chunk schedule)"""
    shape, p, sdf, col, ren = nets
    case = Case(shape.mc, M, "texture")
    default = case.native(sdf, col, torch.ones(M, 1))
    _set_variant(monkeypatch, R, x2h=False)
    mine, ins = run_row(R, nets, M, "texture", "x2h=False", sweeps=False)
    same = all(torch.equal(mine[k], default[1][k]) for k in mine)
    assert not same, "x2h=False changed no gradient: the switch does not reach the direct calls"


RAGGED_SHORT = [33, 97, 2209]


@pytest.mark.parametrize("M", RAGGED_SHORT)
def test_deterministic_variant_on_ragged_rows(R, nets, monkeypatch, M):
    """deterministic=True where M % 32 != 0: the split-K kernels leave through ordered-reduction slabs; twice, bit for bit"""
    assert not PM.runs_x3(M)
    _set_variant(monkeypatch, R, deterministic=True)
    a_leaves, a_ins = run_row(R, nets, M, "texture", "deterministic", sweeps=False)
    shape, p, sdf, col, ren = nets
    _, b_leaves, b_ins = Case(shape.mc, M, "texture").native(sdf, col, torch.ones(M, 1))
    for k in a_leaves:
        assert torch.equal(a_leaves[k], b_leaves[k]), f"deterministic M={M}: {k} differs between two runs"
    for a, b in zip(a_ins, b_ins):
        assert torch.equal(a, b), f"deterministic M={M}: x.grad differs between two runs"


# ------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("step", PM.RENDER_STEPS, ids=[f"{n}x{b}" for n, b, _ in PM.RENDER_STEPS])
def test_render_step_on_a_point_tail(R, step):
    """a train step whose rays x samples is a row-like point count: 33 x 22 = 726 (no multiple of 32), 48 x 22 = 1056,
    40 x 4 = 160.  The rays of tests/shape_matrix.py step_batch's seed; each renders a surface (fp32 oracle: weight_sum
    0.589, 0.439, 0.414)."""
    name, B, batch_step = step
    row = RM.BY_NAME[name]
    shape = SHAPE_BY_NAME[SHAPE]
    lib = R.native.load()
    mc = replace(shape.mc, render=row.render_conf)
    p = live_params(mc, shape.seed)
    sdf, dev, col, ren = R.build_from_named_params(mc, p, device())
    batch = O.synthetic_batch(B, n_lights=row.n_lights, seed=11, step=batch_step, warmup=False)
    M = B * row.S
    stats = {}
    tag = f"render {name} x {B} rays"
    lib.rnb_profile_enable(1)
    try:
        step_against_fp64(R, mc, p, sdf, dev, col, ren, batch, tag, survey=False, stats=stats, loss_rule="calibrated")
        classes = profile_classes(R)
    finally:
        lib.rnb_profile_enable(0)
    assert tuple(ren.last_z_vals.shape) == (B, row.S)
    assert stats["n_checked"] == len(O.param_order(mc))
    assert (FUSED_CLASSES - {X3}) <= classes and ALBEDO_H2_CLASSES <= classes, sorted(classes)
    assert_dw_route(M, classes, tag)
    print(f"POINTROW {tag} M={M} Mp={PM.pad_rows(M)} render: classes {sorted(classes)}; worst output {stats['worst_out'][0]} "
          f"{stats['worst_out'][1]:.2f}, worst gradient {stats['worst_grad'][0]} {stats['worst_grad'][1]:.2f} of its bound")
