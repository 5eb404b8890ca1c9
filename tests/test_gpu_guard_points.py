"""The direct network calls and the sampling entry points between guard bands (tests/guard_bands.py).

The rule of tests/test_gpu_guard_render.py: every call runs once on ordinary allocations and once under guarded() with its
inputs passed through guard(); both bands of every allocation must still hold their pattern, the registry must have seen the
buffers the call is known to make (a workspace of exactly the query that applies, the packed weights and packed_grad, every
output and input-gradient shape), and every result must equal the unguarded run bit for bit.  The bodies of torch.empty
buffers hold the bands' pattern, so a word of a workspace that is read without having been written reads as NaN.  No fp64
oracle is involved.

  1. every row of tests/point_matrix.py through the calls with set_autograd(True), once per backward kind (feature, eikonal,
     color, texture) - the rows and kinds tests/test_gpu_point_matrix.py holds against fp64; the rows whose feature backward
     takes `splits > room` (M = 1056, 8224) are among them;
  2. the no-grad sdf, gradient and color calls at 1, 63 and 4097 points on the shipped shape and on three whose feature width
     is no multiple of 4 (w100, feat1, feat255: the albedo input block then starts and ends off the 16-byte grid);
  3. sample_z_vals, and the up-sampling loop as gpu_support.device_sampling_trace composes it from the per-step entry points.

Not reproducible between two runs of their own: the leaf gradients of the rows with M % 32 != 0, whose weight gradients
leave the split-K kernels through fp32 atomics (tests/point_matrix.py runs_x3 is False there).  Their leaf gradients are
held to "finite exactly where the unguarded run is finite"; their outputs and per-point input gradients are bit-equal like
everything else.  Every case prints one line starting with GUARD."""
import ctypes as C
import time
from dataclasses import replace
from types import SimpleNamespace

import pytest
import torch

from oracle import rnb_oracle as O
from tests import guard_bands as GB
from tests import point_matrix as PM
from tests.field_autograd_util import build, mesh_texture, native_leaf_grads, weights, zero_grads
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device, device_sampling_trace
from tests.shape_matrix import BY_NAME, STEP_RENDER, live_params, points

pytestmark = pytest.mark.gpu

SHAPE = "default_64x64"


@pytest.fixture(scope="module")
def nets(R):
    return build(R, SHAPE)


def _inputs(mc, M, kind):
    """the inputs and adjoint weights of tests/test_gpu_point_matrix.py's Case"""
    F = mc.sdf.d_out - 1
    if kind == "color":
        xs = [points(M, seed=M + 7), torch.nn.functional.normalize(weights(M, 3, 3), dim=-1),
              0.5 * weights(M, mc.color.d_feature, 4)]
    else:
        xs = [points(M, seed=M + {"feature": 0, "eikonal": 5, "texture": 11}[kind])]
    return xs, dict(W1=weights(M, 1, 1), WF=weights(M, F, 2), Wc=weights(M, mc.color.d_out, 5))


def _call(sdf, col, M, kind, xs, w, g):
    zero_grads(sdf, col)
    xs = [g(t.to(device())).requires_grad_(True) for t in xs]
    w = {k: g(v.to(device())) for k, v in w.items()}
    if kind == "feature":
        out = sdf(xs[0])
        loss = (w["W1"] * out[:, :1]).sum() + (w["WF"] * out[:, 1:]).sum()
    elif kind == "eikonal":
        out = sdf.gradient(xs[0]).reshape(M, 3)
        loss = ((out.norm(dim=-1) - 1) ** 2).sum() / M
    elif kind == "color":
        out = col(xs[0], xs[1], xs[1].detach(), xs[2])
        loss = (w["Wc"] * out).sum()
    else:
        out = mesh_texture(sdf, col, xs[0])
        loss = (w["Wc"] * out).sum()
    assert out.grad_fn is not None
    loss.backward()
    torch.cuda.synchronize()
    leaves = {}
    if kind != "color":
        leaves.update(native_leaf_grads(sdf, "sdf"))
    if kind in ("color", "texture"):
        leaves.update(native_leaf_grads(col, "color"))
    assert all(t.grad is not None for t in xs)
    return dict(out=out.detach(), inputs=[t.grad for t in xs]), {k: v for k, v in leaves.items() if v is not None}


def _ws_bytes(R, desc, n, flags=None):
    lib, b = R.native.load(), C.c_int64()
    if flags is None:
        R.native.check(lib.rnb_points_workspace_bytes(C.byref(desc), n, C.byref(b)))
    else:
        R.native.check(lib.rnb_points_grad_workspace_bytes(C.byref(desc), n, flags, C.byref(b)))
    return b.value


def _controls(R, s, sdf, col, M, kind, tag):
    """the buffers each backward kind is known to make"""
    n = R.native
    f32, u8 = torch.float32, torch.uint8
    sdf_desc, col_desc = R.runtime.model_desc(sdf, None), R.runtime._color_desc(col, 256, 6)
    F = sdf_desc.sdf_d_out - 1
    want = []         # (what, shape, dtype, nbytes, at least)
    def ws(what, desc, flags):
        want.append((f"{what} workspace", None, u8, _ws_bytes(R, desc, M, flags), 1))
    def packed(what, desc):
        want.append((f"{what} packed weights + packed_grad", (R.runtime.packed_floats(desc),), f32, None, 2))
    def leaves(what, net):
        want.append((f"{what} flat leaf gradients", (sum(q.numel() for q in net.leaves()),), f32, None, 1))
    if kind in ("feature", "texture"):
        ws("feature", sdf_desc, n.POINTS_FEATURE)
        want += [("sdf", (M, 1), f32, None, 1), ("feature", (M, F), f32, None, 1)]
    if kind in ("eikonal", "texture"):
        ws("normal", sdf_desc, n.POINTS_NORMAL)
        want.append(("normal / x_bar", (M, 3), f32, None, 2))
    if kind != "color":
        packed("sdf", sdf_desc)
        leaves("sdf", sdf)
        want.append(("x_bar", (M, 3), f32, None, 1))
    if kind in ("color", "texture"):
        ws("color", col_desc, n.POINTS_COLOR)
        packed("color", col_desc)
        leaves("color", col)
        want += [("albedo", (M, col_desc.col_d_out), f32, None, 1), ("feat_bar", (M, col_desc.col_d_feature), f32, None, 1),
                 ("pts_bar / nrm_bar", (M, 3), f32, None, 2)]
    for what, shape, dtype, nbytes, least in want:
        got = [e for e in s.seen(shape=shape, dtype=dtype, nbytes=nbytes) if e.how != "guard"]
        assert len(got) >= least, f"{tag}: {what}: {len(got)} guarded allocation(s) of {shape or nbytes}, expected {least}"


@pytest.mark.parametrize("kind", PM.KIND_NAMES)
@pytest.mark.parametrize("row", PM.ROWS, ids=[repr(r) for r in PM.ROWS])
def test_point_row(R, nets, row, kind):
    t0 = time.perf_counter()
    shape, p, sdf, col, ren = nets
    M = row.M
    tag = f"M={M} {kind}"
    xs, w = _inputs(shape.mc, M, kind)
    clean, clean_leaves = _call(sdf, col, M, kind, xs, w, lambda t: t)
    with GB.guarded() as s:
        got, got_leaves = _call(sdf, col, M, kind, xs, w, GB.guard)
        GB.assert_intact(tag)
    _controls(R, s, sdf, col, M, kind, tag)
    GB.assert_same(tag, clean, got)
    rep = PM.runs_x3(M)
    try:
        GB.assert_same(tag + " leaf gradients", clean_leaves, got_leaves, reproducible=rep)
    except AssertionError as e:
        if not rep:
            raise
        _, again = _call(sdf, col, M, kind, xs, w, lambda t: t)
        differ = [k for k in clean_leaves if not GB.same_bits(clean_leaves[k], again[k])]
        raise AssertionError(f"{e}\n  (two unguarded runs differ in {len(differ)} leaf gradients)") from None
    if not rep:        # (printed, not asserted: atomics may agree on one pair of runs)
        _, again = _call(sdf, col, M, kind, xs, w, lambda t: t)
        differ = [k for k in clean_leaves if not GB.same_bits(clean_leaves[k], again[k])]
        print(f"GUARD points {tag}: two unguarded runs differ in {len(differ)} of {len(clean_leaves)} leaf gradients")
    n_alloc = len(s.registry)
    GB.release()
    print(f"GUARD points {tag}: {n_alloc} guarded allocations, {'bit-equal' if rep else 'finite-where-finite'} leaf gradients, "
          f"{time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("n", [1, 63, 4097])
@pytest.mark.parametrize("name", [SHAPE, "w100", "feat1", "feat255"])
def test_no_grad_point_calls(R, name, n):
    """rnb_sdf_forward (with and without the feature), rnb_sdf_gradient and rnb_color_forward on the fused and on the
    per-layer route (w100: padded rows and columns everywhere)"""
    t0 = time.perf_counter()
    shape = BY_NAME[name]
    sdf, devn, col, ren = R.build_from_named_params(shape.mc, live_params(shape.mc, shape.seed), device())
    F = shape.mc.sdf.d_out - 1
    gen = torch.Generator().manual_seed(n + 1)
    ins = dict(pts=points(n, seed=n), nrm=torch.randn(n, 3, generator=gen), feats=torch.randn(n, F, generator=gen) * 0.3)
    desc = R.model_desc(sdf, col)

    @torch.no_grad()
    def call(g):
        x = {k: g(v.to(device())) for k, v in ins.items()}
        packed = R.runtime.pack_weights(desc, sdf, col, device())
        res = dict(full=R.runtime.sdf_forward(desc, packed, x["pts"], True), only=R.runtime.sdf_forward(desc, packed, x["pts"], False),
                   grad=R.runtime.sdf_gradient(desc, packed, x["pts"]),
                   alb=R.runtime.color_forward(desc, packed, x["pts"], x["nrm"], x["feats"]),
                   direct_sdf=sdf.sdf(x["pts"]), direct_grad=sdf.gradient(x["pts"]), direct_col=col(x["pts"], x["nrm"], x["nrm"], x["feats"]))
        torch.cuda.synchronize()
        return res

    tag = f"no-grad {name} n={n}"
    clean = call(lambda t: t)
    with GB.guarded() as s:
        got = call(GB.guard)
        GB.assert_intact(tag)
    ws = _ws_bytes(R, desc, n)
    assert len(s.seen(nbytes=ws, dtype=torch.uint8)) >= 4, f"{tag}: four calls, each with a workspace of rnb_points_workspace_bytes = {ws}"
    assert s.seen(shape=(R.runtime.packed_floats(desc),), dtype=torch.float32)
    for shp in ((n, 1), (n, F), (n, 3), (n, shape.mc.color.d_out)):
        assert [e for e in s.seen(shape=shp, dtype=torch.float32) if e.how != "guard"], f"{tag}: no guarded output {shp}"
    GB.assert_same(tag, clean, got)
    print(f"GUARD points {tag}: {len(s.registry)} guarded allocations, {time.perf_counter() - t0:.2f} s")
    GB.release()


# ------------------------------------------------------------------------------------------------------------------- 3
SAMPLING = [("default_64x64", None, 37), ("default_64x64", STEP_RENDER, 37), ("default_64x64", O.RenderConf(n_samples=65, n_importance=64, up_sample_steps=1), 5),
            ("default_64x64", O.RenderConf(n_samples=64, n_importance=448, up_sample_steps=7), 5), ("w32", O.RenderConf(n_samples=17, n_importance=5, up_sample_steps=1), 5),
            ("w32", O.RenderConf(n_samples=2, n_importance=0, up_sample_steps=1), 3)]


@pytest.mark.parametrize("case", SAMPLING, ids=[f"{n}-{'own' if rc is None else f'{rc.n_samples}+{rc.n_importance}'}-B{B}" for n, rc, B in SAMPLING])
def test_sampling_entry_points(R, case):
    """rnb_sample_rays (sample_z_vals) and the same loop composed from rnb_up_sample_step, rnb_sdf_forward and rnb_gather_sdf"""
    t0 = time.perf_counter()
    name, rc, B = case
    shape = BY_NAME[name]
    mc = shape.mc if rc is None else replace(shape.mc, render=rc)
    rc = mc.render
    sdf, devn, col, ren = R.build_from_named_params(mc, live_params(mc, shape.seed), device())
    ren0 = R.NeuSRenderer(None, sdf, devn, col, n_samples=rc.n_samples, n_importance=0, n_outside=0, up_sample_steps=1,
                          perturb=rc.perturb)
    batch = O.synthetic_batch(B, seed=11, step=1)

    @torch.no_grad()
    def call(g):
        b = {k: g(batch[k].to(device())) for k in ("rays_o", "rays_d", "near", "far", "t_rand")}
        packed = ren._pack(False)
        z = ren.sample_z_vals(b["rays_o"], b["rays_d"], b["near"], b["far"], packed, 1.0, b["t_rand"])
        z0 = ren0.sample_z_vals(b["rays_o"], b["rays_d"], b["near"], b["far"], packed, 1.0, b["t_rand"])
        res = dict(z=z, z0=z0)
        if rc.n_importance > 0:
            inds, zc = device_sampling_trace(R, SimpleNamespace(mc=mc), sdf, b, z0)
            res.update(inds=inds, z_composed=zc)
        torch.cuda.synchronize()
        return res

    tag = f"sampling {name} {rc.n_samples}+{rc.n_importance}/{rc.up_sample_steps} B={B}"
    clean = call(lambda t: t)
    with GB.guarded() as s:
        got = call(GB.guard)
        GB.assert_intact(tag)
    lib, nb = R.native.load(), C.c_int64()
    R.native.check(lib.rnb_sample_workspace_bytes(C.byref(ren.desc), B, C.byref(nb)))
    assert s.seen(nbytes=max(nb.value, 256), dtype=torch.uint8), f"{tag}: no workspace of rnb_sample_workspace_bytes = {nb.value}"
    S = rc.n_samples + rc.n_importance
    assert s.seen(shape=(B, S), dtype=torch.float32) and s.seen(shape=(B, rc.n_samples), dtype=torch.float32)
    if rc.n_importance > 0:
        n_new = rc.n_importance // rc.up_sample_steps
        assert s.seen(shape=(B, n_new), dtype=torch.int32) and s.seen(shape=(B, S), dtype=torch.int32), f"{tag}: per-step outputs"
        assert torch.equal(got["z"], got["z_composed"]), f"{tag}: rnb_sample_rays and the composed loop differ"
    GB.assert_same(tag, clean, got)
    print(f"GUARD points {tag}: {len(s.registry)} guarded allocations, {time.perf_counter() - t0:.2f} s")
    GB.release()
