"""The zero-tile path of the fused albedo backward (csrc/color_h2.hip): a 64-point tile whose colour adjoint is
exactly zero — every ray in it lies outside the mask — is skipped by the albedo backward (no product runs; its zc_l / cinb rows
stay unwritten), by FB's feature-head seed and by the weight-gradient jobs that read those rows (where the weight gradients go
to kernels that read every row, the tile stores zeros instead).  The contract is exactness: skipping on and
RNB_VARIANT_NO_DEAD_TILES (`set_variant(dead_tiles=False)`) give equal outputs and equal gradients (-0 equals +0), NaN for NaN.

Full-size networks (the `full_main_sharp` state) on three small point counts:
  B = 8, S = 128   16 tiles, rays aligned to tiles (a ray is two tiles)
  B = 6, S = 96    576 points, 9 tiles: tiles straddle rays, a tile is dead only if both its rays are
  B = 3, S = 80    240 points, 4 tiles: the last one has 16 padding rows (240 is no multiple of 32: the weight gradients go
                   to the split-K kernels)
and five masks: all in, all out, alternating, one ray in, one ray out.  The depths are explicit (tests/gpu_support.py
explicit_depths), so both variants render the same points.

The number of tiles skipped is held to a count made on the CPU.  A tile is dead when the colour adjoint of each of its real
points is exactly zero, and a point's colour adjoint is (the ray's dcolor) x (the point's compositing weight): zero when the
ray is outside the mask, and also when the weight is exactly zero — behind the sharp surface of this state alpha is exactly 0.
The mask and the tile map alone give a LOWER bound (3 of 9 tiles for the alternating mask at B = 6, where the device skips 4:
measured on MI355X); the count asserted is made from the mask, the tile map and the `weights` the render itself returned.  By
the mask alone no tile of the 240-point shape is free of rays 0 and 2, so "alternating" and "one ray out" need not skip any
tile there."""
import dataclasses

import pytest
import torch

from oracle import rnb_oracle as O
from tests import gpu_support as G
from tests.golden_util import Golden
from tests.gpu_support import R, device  # noqa: F401  (R: the module-scoped fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(8, 128), (6, 96), (3, 80)]
MASKS = ["all_in", "all_out", "alternating", "one_in", "one_out"]


def make_mask(kind, B):
    m = torch.zeros(B, 1)
    if kind == "all_in":
        m[:] = 1.0
    elif kind == "alternating":
        m[0::2] = 1.0
    elif kind == "one_in":
        m[B // 2] = 1.0
    elif kind == "one_out":
        m[:] = 1.0
        m[B // 2] = 0.0
    else:
        assert kind == "all_out", kind
    return m


def dead_tiles_expected(mask, B, S, weights=None):
    """tiles of 64 consecutive points (point i is sample i % S of ray i // S) none of whose real points carries a colour
    adjoint: its ray is outside the mask or (with `weights` [B, S], the render's own) its compositing weight is exactly zero"""
    M = B * S
    live = (mask.reshape(B, 1) != 0).expand(B, S)
    if weights is not None:
        live = live & (weights.reshape(B, S).cpu() != 0)
    live = live.reshape(-1)
    return sum(int(not bool(live[64 * t:min(M, 64 * t + 64)].any())) for t in range((M + 63) // 64))


class Scene:
    """the device modules of full_main_sharp at one (B, S), with one batch and its explicit depths"""

    def __init__(self, R, B, S):
        g = Golden("full_main_sharp")
        self.mc = dataclasses.replace(g.mc, render=dataclasses.replace(g.mc.render, n_samples=S // 2, n_importance=S // 2))
        self.p = g.params()
        self.sdf, self.dev, self.col, self.ren = R.build_from_named_params(self.mc, self.p, device())
        self.B, self.S = B, S
        # (seeds whose rays hit the surface: tests/gpu_support.py assert_has_surface)
        self.batch = O.synthetic_batch(B, seed={128: 14}.get(S, 11), step=S)
        self.z = G.explicit_depths(self.batch, S, seed=S)
        self.R = R

    def params(self):
        return G.named(self.sdf, self.dev, self.col)

    def step(self, mask, dead_tiles=True, count=False, **variant):
        """one train-shaped step -> (outputs, gradients by name, dead tiles reported or None)"""
        b = {k: v.to(device()) for k, v in self.batch.items()}
        m = mask.to(device())
        for q in self.params().values():
            q.grad = None
        self.ren.set_variant(dead_tiles=dead_tiles, **variant)
        self.ren.track_range = count
        try:
            out = self.ren.render_rnb(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=1.0,
                                      z_vals=self.z.to(device()))
            loss = self.R.rnb_loss(out, b["true_rgb"], m)[0]
            loss.backward()
            torch.cuda.synchronize()
            n_dead = self.ren.range_report()["dead_tiles"] if count else None
        finally:
            self.ren.track_range = False
            self.ren.set_variant()
        outs = {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}
        outs["loss"] = loss.detach().clone()
        return outs, {k: v.grad.detach().clone() for k, v in self.params().items()}, n_dead


_SCENES = {}


@pytest.fixture(scope="module")
def scene(R):
    def get(B, S):
        if (B, S) not in _SCENES:
            _SCENES[(B, S)] = Scene(R, B, S)
        return _SCENES[(B, S)]
    yield get
    _SCENES.clear()


def assert_same(a, b, what):
    """numpy.array_equal with NaN for NaN: the same NaN pattern and equal finite elements (-0 equals +0)"""
    for k in a:
        x, y = a[k], b[k]
        nx, ny = torch.isnan(x), torch.isnan(y)
        assert torch.equal(nx, ny), f"{what}: {k}: NaN pattern differs"
        assert torch.equal(x[~nx], y[~ny]), f"{what}: {k}: max |d| {float((x[~nx] - y[~ny]).abs().max()):.3e}"


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("B,S", SHAPES)
def test_skipping_equals_the_full_path(scene, B, S, kind):
    sc = scene(B, S)
    mask = make_mask(kind, B)
    by_mask = dead_tiles_expected(mask, B, S)
    o1, g1, n1 = sc.step(mask, dead_tiles=True, count=True)
    o0, g0, n0 = sc.step(mask, dead_tiles=False, count=True)
    want = dead_tiles_expected(mask, B, S, o1["weights"])
    print(f"B {B} S {S} {kind}: dead tiles {n1} of {(B * S + 63) // 64}; CPU count {want} (by the mask alone {by_mask}); "
          f"full path reports {n0}")
    assert n1 == want, f"{n1} tiles skipped, {want} carry no colour adjoint"
    assert n1 >= by_mask
    assert n0 == 0
    if kind == "all_in":
        assert by_mask == 0
    elif not (S == 80 and kind in ("alternating", "one_out")):
        assert by_mask > 0 and n1 > 0
    assert_same(o1, o0, "output")
    assert_same(g1, g0, "gradient")
    assert all(bool(torch.isfinite(v).all()) for v in g1.values())
    # the albedo network still learns from the rays in the mask; the SDF network from every ray
    if kind != "all_out":
        assert float(g1["color.lin0.weight_v"].abs().max()) > 0
    assert float(g1["sdf.lin0.weight_v"].abs().max()) > 0


@pytest.mark.parametrize("B,S", SHAPES)
def test_masked_step_against_fp64(scene, B, S):
    """tests/gpu_support.py step_against_fp64 at the golden bounds, alternating mask, skipping on (the default)"""
    sc = scene(B, S)
    batch = dict(sc.batch, mask=make_mask("alternating", B))
    for q in sc.params().values():
        q.grad = None
    G.step_against_fp64(sc.R, sc.mc, sc.p, sc.sdf, sc.dev, sc.col, sc.ren, batch, f"dead_tiles B{B} S{S}", survey=False, z_vals=sc.z)


@pytest.mark.parametrize("B,S,kind", [(6, 96, "alternating"), (3, 80, "one_in")])
def test_unwritten_dead_tile_buffers_are_never_read(R, B, S, kind):
    """The method of tests/test_gpu_parity.py test_uninitialised_workspace_is_never_read with a masked batch: a dead tile runs
    none of the products that fill zc_l and cinb, so a row it failed to store as zeros, or a reader of what it leaves
    unwritten (cinb's encoding columns, the slabs), would pick up the NaN patterns the buffers are pre-filled with.  240 points:
    the last tile has padding rows."""
    runs = []
    orig_empty, orig_empty_like = torch.empty, torch.empty_like

    def poison(t):
        if t.is_cuda and t.dtype == torch.float32:
            t.fill_(float("nan"))
        elif t.is_cuda and t.dtype == torch.uint8:
            t.fill_(255)
        return t

    mask = make_mask(kind, B)
    for poisoned in (False, True):
        sc = Scene(R, B, S)
        if poisoned:
            torch.empty = lambda *a, **k: poison(orig_empty(*a, **k))
            torch.empty_like = lambda *a, **k: poison(orig_empty_like(*a, **k))
        try:
            runs.append(sc.step(mask, dead_tiles=True, count=True, deterministic=True))
        finally:
            torch.empty, torch.empty_like = orig_empty, orig_empty_like
    (o0, g0, n0), (o1, g1, n1) = runs
    assert n0 == n1 and n0 >= dead_tiles_expected(mask, B, S) > 0
    for k in o0:
        assert torch.equal(o0[k], o1[k]), f"output {k} depends on what its buffers held before the call"
    for k in g0:
        assert torch.equal(g0[k], g1[k]), f"gradient of {k} depends on what the workspace held before the call"


@pytest.mark.parametrize("what", ["inf_hidden_bias", "nan_weight_v", "inf_output_weight"])
def test_non_finite_parameters_keep_their_nans(R, what):
    """0 x inf and 0 x NaN are NaN in the reference: a tile whose skipped products would meet a non-finite operand takes the
    full path.  Skipping on equals the full path in NaN pattern and in every finite element; no fault; no tile is skipped.
    The first two cases reach the forward's launch-level word (a non-finite activation); an infinite row of W_out leaves the
    hidden activations finite and is caught in the backward kernel itself (W_out and the albedo are checked there)."""
    B, S = 8, 128
    sc = Scene(R, B, S)
    with torch.no_grad():
        if what == "inf_hidden_bias":
            sc.col.lin1.bias[5] = float("inf")
        elif what == "inf_output_weight":
            sc.col.lin2.weight_g[1] = float("inf")
        else:
            sc.col.lin1.weight_v[3, 7] = float("nan")
    mask = make_mask("alternating", B)
    o1, g1, n1 = sc.step(mask, dead_tiles=True, count=True)
    o0, g0, _ = sc.step(mask, dead_tiles=False)
    print(f"{what}: dead tiles {n1}; NaN gradient tensors {sum(int(bool(torch.isnan(v).any())) for v in g0.values())} of {len(g0)}")
    assert n1 == 0, f"{n1} tiles skipped although an operand of the skipped products is not finite"
    assert_same(o1, o0, "output")
    assert_same(g1, g0, "gradient")
    assert any(bool(torch.isnan(v).any()) for v in g0.values()), "the case must reach a NaN in the full path"


def test_masked_gradients_are_bit_reproducible(scene):
    """three runs of the masked step: the live tiles are walked in ascending order, so the sums depend on the inputs alone"""
    sc = scene(6, 96)
    mask = make_mask("alternating", 6)
    runs = [sc.step(mask)[1] for _ in range(3)]
    for r in runs[1:]:
        for k in runs[0]:
            assert torch.equal(runs[0][k], r[k]), k
