"""Drop-in NeuSRenderer (models/renderer.py:72-1224) backed by librnbneus_hip.so.

Same constructor, same `render`, `render_rnb`, `render_rnb_warmup`, `extract_geometry` signatures and
the same dict of tensors (models/renderer.py:638-648, :920-930, :1023-1033).  The returned tensors are
attached to autograd through one torch.autograd.Function whose backward runs the native explicit
backward (rnb_render_bwd + rnb_weightnorm_bwd) and returns `.grad`s for every trainable leaf, so the
reference's `loss.backward(); optimizer.step()` (exp_runner.py:259-263) works unchanged.

Differences that are deliberate and documented in DESIGN.md:
  * n_outside must be 0 (every shipped config); the NeRF background path is not implemented.
  * the [B,1] perturbation draw (renderer.py:572) is made here with torch.rand on the rays' device and
    may be supplied explicitly (`t_rand=`) so that tests can feed the oracle the same randomness.
  * with data parallelism enabled (`set_data_parallel`) the backward all-reduces the flat gradient
    buffer over RCCL before returning.  Default `exact=True`: the ranks hold contiguous shards of ONE global
    batch; the render returns its shard's eikonal sums (models/renderer.py:538-540) on a token attached to
    `gradient_error`, `rnb_loss(..., group=)` all-reduces them TOGETHER with `mask_sum` / the ray count in one
    4-float collective, and the gradient all-reduce is a SUM, so a G-rank step equals the single-process step
    on the whole batch.  Forwards are never collective (a rank-0-only validation render cannot desynchronise
    the ranks); the collectives of a step are the loss's and the backward's, and the backward raises if the
    loss it is driven by was not `rnb_loss(..., group=)`.  `exact=False` is the DDP convention (per-rank
    normalisers, mean of the per-rank gradients, any loss).
  * kernel / arithmetic variants (`set_variant`): explicit bits of the model descriptor, no environment
    variables (bf16 sweeps for BASELINE config 5, deterministic reductions, A/B tuning knobs).
"""
from __future__ import annotations

import ctypes as C
import logging

import numpy as np
import torch
import torch.distributed as dist

from . import mesh_pipeline, native, parallel, runtime
from .fields import mlp_struct, model_desc
from .parallel import allreduce_mean_, allreduce_sum_

_MESH_BACKEND_LOGGED = False
# cells per brick edge of extract_fields_sparse(brick=None): chosen from profiles/sparse_grid.txt
DEFAULT_SPARSE_BRICK = 8


# whole-image rendering (render_maps / render_image)
_MAPS_API = {"render": native.MODE_CORE, "render_rnb": native.MODE_MVPS,
             "render_rnb_warmup": native.MODE_MVPS | native.FLAG_RELU_SHADING}
_MAPS_KNOWN = ("color", "normal", "albedo", "depth", "weight_sum", "weight_max")
DEFAULT_MAPS = ("color", "normal", "albedo", "depth", "weight_sum")
# rays per launch of a whole-image render: where profiles/image_render.txt shows the throughput flatten
DEFAULT_CHUNK_RAYS = 1024


def _requires_grad(t):
    return isinstance(t, torch.Tensor) and t.requires_grad


class ExactDPToken:
    """Travels on `out["gradient_error"]` of a render made under grad in exact data-parallel mode.  Carries this
    shard's eikonal (numerator, count) to `rnb_loss(..., group=)`, which all-reduces them with the mask counts, writes
    the global denominator into `gerr_den_global` (read by the native backward) and marks the token paired."""

    def __init__(self, group, gerr_partial, gerr_den_global):
        self.group, self.gerr_partial, self.gerr_den_global = group, gerr_partial, gerr_den_global
        self.paired = False

_OUT_KEYS = ("color_fine", "s_val", "cdf_fine", "weight_sum", "weight_max", "gradients", "weights",
             "gradient_error", "inside_sphere")


_N_INPUTS = 5   # rays_o, rays_d, lights, background_rgb, z_vals: the differentiable inputs of _FinePass, before the leaves


class _ZFromNearFar(torch.autograd.Function):
    """n_importance == 0: z = near + (far - near) t_s (+ the perturbation) as the native sampler computed it (models/renderer.py
    :560-572).  The forward returns those z unchanged (no recomputation in torch: their bits stay the sampler's); the
    backward is near_bar = sum_s z_bar (1 - t_s), far_bar = sum_s z_bar t_s."""

    @staticmethod
    def forward(ctx, near, far, z):
        ctx.shapes = (getattr(near, "shape", None), getattr(far, "shape", None))
        return z.clone()

    @staticmethod
    def backward(ctx, zbar):
        if zbar is None:
            return None, None, None
        t = torch.linspace(0.0, 1.0, zbar.shape[1], device=zbar.device, dtype=torch.float32)
        near_bar = (zbar * (1.0 - t)).sum(-1).reshape(ctx.shapes[0]) if ctx.needs_input_grad[0] else None
        far_bar = (zbar * t).sum(-1).reshape(ctx.shapes[1]) if ctx.needs_input_grad[1] else None
        return near_bar, far_bar, None


class _FinePass(torch.autograd.Function):
    """forward: rnb_weightnorm_fwd (done by the caller) + rnb_render_fwd; backward: rnb_render_bwd +
    rnb_weightnorm_bwd (+ optional RCCL all-reduce of the flat gradient buffer).  With an input that requires grad
    (rays_o, rays_d, lights, background_rgb, z_vals; RNB_FLAG_INPUT_GRADS in the forward) the backward is
    rnb_render_bwd_inputs, which also writes those inputs' gradients (shard-local: never all-reduced)."""

    @staticmethod
    def forward(ctx, renderer, call, rays_o, rays_d, lights, bg, z, *leaves):
        lib = native.load()
        desc = renderer.desc
        dev = call["rays_o"].device
        B, S = call["z_vals"].shape
        flags = call["flags"]
        mvps = bool(flags & native.MODE_MVPS)
        L = call["lights"].shape[0] if mvps else 1
        Cd = desc.col_d_out
        f32 = dict(dtype=torch.float32, device=dev)
        out = {
            "color_fine": torch.empty((L, B, Cd) if mvps else (B, 3), **f32),
            "weights": torch.empty(B, S, **f32),
            "cdf_fine": torch.empty(B, S, **f32),
            "gradients": torch.empty(B, S, 3, **f32),
            "inside_sphere": torch.empty(B, S, **f32),
            "weight_sum": torch.empty(B, 1, **f32),
            "weight_max": torch.empty(B, 1, **f32),
            "s_val": torch.empty(B, 1, **f32),
            "gradient_error": torch.empty((), **f32),
        }
        extras = {}
        if call.get("want_extras"):
            extras["sdf"] = torch.empty(B * S, 1, **f32)
            if not (mvps and (flags & native.FLAG_NO_ALBEDO)):
                extras["sampled_albedo"] = torch.empty(B, S, Cd, **f32)
        ws = native.workspace("render", dev, C.byref(desc), B, S, flags)
        args = native.RenderArgs()
        args.B, args.S, args.n_lights, args.flags = B, S, L, flags
        args.cos_anneal_ratio = float(call["cos_anneal_ratio"])
        keep = dict(rays_o=call["rays_o"], rays_d=call["rays_d"], z_vals=call["z_vals"], lights=call["lights"],
                    bg=call["background_rgb"], variance=renderer.deviation_network.variance.detach().reshape(1))
        args.rays_o, args.rays_d = keep["rays_o"].data_ptr(), keep["rays_d"].data_ptr()
        args.z_vals = keep["z_vals"].data_ptr()
        args.lights_dir = keep["lights"].data_ptr() if keep["lights"] is not None else None
        args.background_rgb = keep["bg"].data_ptr() if keep["bg"] is not None else None
        args.variance = keep["variance"].data_ptr()
        for k in ("color_fine", "weights", "cdf_fine", "gradients", "inside_sphere", "weight_sum", "weight_max",
                  "s_val", "gradient_error"):
            setattr(args, k, out[k].data_ptr())
        args.sdf = extras["sdf"].data_ptr() if "sdf" in extras else None
        args.sampled_albedo = extras["sampled_albedo"].data_ptr() if "sampled_albedo" in extras else None
        # exact data parallel, training render: keep this shard's eikonal (numerator, count); the loss all-reduces them
        # (no collective here: forwards stay local, forward-only renders return the shard-local gradient_error)
        exact_dp = renderer.dp_group is not None and renderer.dp_exact and not (flags & native.FLAG_FORWARD_ONLY)
        ctx.dp_token = None
        if exact_dp:
            keep["gerr_partial"] = torch.empty(2, **f32)
            keep["gerr_den_global"] = torch.empty(1, **f32)
            args.gerr_partial = keep["gerr_partial"].data_ptr()
            args.gerr_den_global = keep["gerr_den_global"].data_ptr()
            ctx.dp_token = ExactDPToken(renderer.dp_group, keep["gerr_partial"], keep["gerr_den_global"])
        with native.on_device(dev) as stream:
            native.check(lib.rnb_render_fwd(C.byref(desc), native.ptr(call["packed"]), C.byref(args), native.ptr(ws),
                                            ws.numel(), stream))
        if renderer.track_range and (flags & native.FLAG_FORWARD_ONLY):
            renderer._collect_range(desc, call["packed"], ws, B, S, flags)
        ctx.renderer, ctx.call, ctx.args, ctx.keep, ctx.ws, ctx.out = renderer, call, args, keep, ws, out
        # the descriptor AS OF this forward: the backward must carve the workspace with the layout the forward wrote,
        # whatever set_variant() did in between
        ctx.desc = native.ModelDesc.from_buffer_copy(desc)
        ctx.dp = (renderer.dp_group, renderer.dp_exact)
        ctx.n_leaves = len(leaves)
        ctx.mark_non_differentiable(out["inside_sphere"])
        # outputs the loss does not touch arrive as None in backward (no zero tensors are materialised;
        # the native backward treats a NULL cotangent as zero)
        ctx.set_materialize_grads(False)
        renderer.last_extras = extras
        renderer._last_dp_token = ctx.dp_token
        return tuple(out[k] for k in _OUT_KEYS)

    @staticmethod
    def backward(ctx, *gouts):
        lib = native.load()
        renderer, call, desc = ctx.renderer, ctx.call, ctx.desc
        dp_group, dp_exact = ctx.dp
        if ctx.ws is None:
            raise RuntimeError("NeuSRenderer: backward called a second time on the same render (the saved per-point "
                               "state is released after the first backward, retain_graph is not supported); re-run "
                               "the forward")
        if ctx.dp_token is not None and not ctx.dp_token.paired:
            raise RuntimeError("NeuSRenderer: exact data-parallel mode (set_data_parallel(exact=True)) needs the loss to "
                               "be rnb_loss(..., group=<the data-parallel group>): it all-reduces the batch-global "
                               "normalisers this backward divides by.  Use set_data_parallel(exact=False) with any "
                               "other loss (DDP mean of per-rank gradients)")
        dev = ctx.ws.device
        g = dict(zip(_OUT_KEYS, gouts))
        keepalive = []

        def gp(name):
            t = g.get(name)
            if t is None:
                return None
            t = t.to(torch.float32).contiguous()
            keepalive.append(t)
            return t.data_ptr()

        rg = native.RenderGrads()
        for k in ("color_fine", "weights", "cdf_fine", "gradients", "weight_sum", "weight_max", "s_val",
                  "gradient_error"):
            setattr(rg, k, gp(k))
        packed_grad = torch.empty_like(call["packed"])
        flat, views, order = renderer._alloc_flat_grads(call["train_color"], dev)
        dvar = views[id(renderer.deviation_network.variance)]
        # input gradients (float32, the shapes handed to the forward; autograd maps them back to the caller's through the
        # differentiable .to() / reshape of _run)
        want = ctx.needs_input_grad[2:2 + _N_INPUTS]
        in_grads = [None] * _N_INPUTS
        ig = None
        if any(want):
            ig = native.RenderInputGrads()
            for i, (name, src) in enumerate((("rays_o", call["rays_o"]), ("rays_d", call["rays_d"]),
                                             ("lights_dir", call["lights"]), ("background_rgb", call["background_rgb"]),
                                             ("z_vals", call["z_vals"]))):
                if want[i]:
                    in_grads[i] = torch.empty(src.shape, dtype=torch.float32, device=dev)
                    setattr(ig, name, in_grads[i].data_ptr())
        with native.on_device(dev) as stream:
            if ig is None:
                native.check(lib.rnb_render_bwd(C.byref(desc), native.ptr(call["packed"]), C.byref(ctx.args),
                                                C.byref(rg), native.ptr(packed_grad), C.c_void_p(dvar.data_ptr()),
                                                native.ptr(ctx.ws), ctx.ws.numel(), stream))
            else:
                native.check(lib.rnb_render_bwd_inputs(C.byref(desc), native.ptr(call["packed"]), C.byref(ctx.args),
                                                       C.byref(rg), C.byref(ig), native.ptr(packed_grad),
                                                       C.c_void_p(dvar.data_ptr()), native.ptr(ctx.ws), ctx.ws.numel(),
                                                       stream))
        if renderer.track_range:
            renderer._collect_range(desc, call["packed"], ctx.ws, ctx.args.B, ctx.args.S, ctx.args.flags)
        sdf_net, col_net = renderer.sdf_network, renderer.color_network
        sp = mlp_struct(sdf_net.lins(), sdf_net.weight_norm)
        sg = mlp_struct(sdf_net.lins(), sdf_net.weight_norm, grads=views)
        use_col = call["train_color"]
        cp = mlp_struct(col_net.lins(), col_net.weight_norm) if use_col else None
        cg = mlp_struct(col_net.lins(), col_net.weight_norm, grads=views) if use_col else None
        with native.on_device(dev) as stream:
            native.check(lib.rnb_weightnorm_bwd(C.byref(desc), C.byref(sp), C.byref(cp) if cp is not None else None,
                                                native.ptr(packed_grad), C.byref(sg),
                                                C.byref(cg) if cg is not None else None, stream))
        if dp_group is not None:
            # the one exchange step of the path: the flat gradient buffer over xGMI (RCCL).  exact: the per-rank
            # losses are additive shares of the whole batch's loss -> SUM; otherwise the DDP mean.
            if dp_exact:
                allreduce_sum_(flat, dp_group)
            else:
                allreduce_mean_(flat, dp_group)
        ctx.ws = None
        grads = []
        for i, leaf in enumerate(call["leaves"]):
            v = views.get(id(leaf))
            grads.append(v.view_as(leaf) if v is not None and ctx.needs_input_grad[2 + _N_INPUTS + i] else None)
        return (None, None) + tuple(in_grads) + tuple(grads)


class NeuSRenderer:
    def __init__(self, nerf, sdf_network, deviation_network, color_network, n_samples, n_importance, n_outside,
                 up_sample_steps, perturb):
        if n_outside != 0:
            raise NotImplementedError("n_outside > 0 (NeRF background) is outside the accelerated path; every "
                                      "shipped config uses n_outside = 0")
        self.nerf = nerf
        self.sdf_network = sdf_network
        self.deviation_network = deviation_network
        self.color_network = color_network
        self.n_samples = n_samples
        self.n_importance = n_importance
        self.n_outside = n_outside
        self.up_sample_steps = up_sample_steps
        self.perturb = perturb
        # the reference reads self.color_depth without ever setting it (renderer.py:226; patched from
        # outside at exp_runner.py:125) — default it from the albedo network
        # (color_network None: a geometry-only renderer — extract_geometry, vertex_attributes without albedo)
        self.color_depth = color_network.d_out if color_network is not None else None
        self.desc = model_desc(sdf_network, color_network, n_samples, n_importance, up_sample_steps)
        self.dp_group = None
        self.dp_exact = True
        self.last_z_vals = None
        self.last_extras = {}
        self.want_extras = False
        # diagnostics: with track_range the largest operand magnitudes of every render are read back (rnb_render_range: one
        # more pass over the saved state per step — off by default); range_report() returns the last ones
        self.track_range = False
        self._range = None
        self.last_sparse_grid = None   # `info` of the last extract_geometry(sparse=True)
        self.last_mesh_clean = None    # `info` of the last extract_geometry / extract_textured_geometry(clean=...)
        self.last_mesh_simplify = None  # `info` of the last extract_geometry / extract_textured_geometry(simplify=...)
        self.last_mesh_cull = None     # `info` of the last extract_geometry / extract_textured_geometry(cull=...)
        self.last_mesh_fill = None     # `info` of the last extract_geometry / extract_textured_geometry(fill=...)

    # ------------------------------------------------------------------ data parallel
    def set_data_parallel(self, group=None, enabled=True, exact=True):
        """One process per GPU, each rendering its contiguous shard of a global ray batch; the backward
        all-reduces the flat gradient buffer over `group` — BACKWARDS are collective, forwards never are (a
        forward-only / no_grad render on one rank alone is fine and returns the shard-local `gradient_error`).
        exact=True (default): large-batch semantics, see the module docstring; the loss MUST then be
        `rnb_loss(..., group=group)` — the pairing is checked both ways (the backward raises otherwise, and so does
        `rnb_loss(group=)` on a render that was not made in exact mode).  exact=False: DDP mean of per-rank
        gradients, per-rank normalisers, any loss (`rnb_loss` without a group, or the reference's torch ops).
        Gradients of the render's inputs (rays, lights, background, z) are shard-local and never all-reduced, as DDP treats
        non-parameter tensors: in exact mode a rank's per-ray rows equal the single-process rows, and the single-process
        gradient of a replicated input (shared lights, the background) is the sum over the ranks."""
        self.dp_group = (group if group is not None else dist.group.WORLD) if enabled else None
        self.dp_exact = bool(exact)

    def set_variant(self, **kw):
        """Kernel / arithmetic variant bits of the model descriptor (include/rnbneus.h RNB_VARIANT_*):
        bf16=, deterministic=, generic=, dw_lds=, bwd_ti=, bwd_nw=, fwd_ti=, fwd_nw=, dead_tiles=.  Returns self."""
        self.desc.variant = native.variant_bits(**kw)
        return self

    # ------------------------------------------------------------------ helpers
    def _leaves(self, train_color):
        leaves = list(self.sdf_network.leaves()) + [self.deviation_network.variance]
        if train_color:
            leaves += list(self.color_network.leaves())
        return leaves

    def _alloc_flat_grads(self, train_color, dev):
        leaves = self._leaves(train_color)
        total = sum(p.numel() for p in leaves)
        flat = torch.empty(total, dtype=torch.float32, device=dev)
        views, off = {}, 0
        for p in leaves:
            views[id(p)] = flat[off:off + p.numel()]
            off += p.numel()
        return flat, views, leaves

    def _pack(self, use_color):
        dev = self.sdf_network.lin0.bias.device
        return runtime.pack_weights(self.desc, self.sdf_network, self.color_network if use_color else None, dev)

    def sample_z_vals(self, rays_o, rays_d, near, far, packed, perturb, t_rand=None):
        """The no-grad prologue shared by the three wrappers (models/renderer.py:557-608)."""
        lib = native.load()
        B = rays_o.shape[0]
        dev = rays_o.device
        if perturb > 0:
            if t_rand is None:
                t_rand = torch.rand([B, 1], device=dev)
            t_rand = t_rand.to(torch.float32).reshape(B).contiguous()
        else:
            t_rand = None
        S = self.n_samples + self.n_importance
        z = torch.empty(B, S, dtype=torch.float32, device=dev)
        ws = native.workspace("sample", dev, C.byref(self.desc), B, floor=256)
        near = near.to(torch.float32).reshape(B).contiguous()
        far = far.to(torch.float32).reshape(B).contiguous()
        native.same_device(packed, rays_o, rays_d, near, far, t_rand)
        with native.on_device(dev) as stream:
            native.check(lib.rnb_sample_rays(C.byref(self.desc), native.ptr(packed), native.ptr(rays_o),
                                             native.ptr(rays_d), native.ptr(near), native.ptr(far), native.ptr(t_rand),
                                             B, native.ptr(z), native.ptr(ws), ws.numel(), stream))
        return z

    def _run(self, rays_o, rays_d, near, far, lights_dir, perturb_overwrite, background_rgb, cos_anneal_ratio,
             flags, t_rand, z_vals):
        if not rays_o.is_cuda:
            raise RuntimeError("NeuSRenderer: rays must be on the GPU (no CPU path; librnbneus_hip.so only)")
        dev = rays_o.device
        if self.sdf_network.lin0.bias.device != dev:
            raise RuntimeError(f"NeuSRenderer: rays live on {dev} but the networks on "
                               f"{self.sdf_network.lin0.bias.device}")
        B = rays_o.shape[0]
        mvps = bool(flags & native.MODE_MVPS)
        no_albedo = bool(flags & native.FLAG_NO_ALBEDO)
        use_color = not (mvps and no_albedo)
        # inputs the caller's graph differentiates (the reference's autograd reaches each of them): rays, lights (render_rnb*),
        # the background (render) and z (given, or near / far with n_importance == 0: models/renderer.py:560, :590)
        grad_enabled = torch.is_grad_enabled()
        z_req = _requires_grad(z_vals) if z_vals is not None else (
            self.n_importance == 0 and (_requires_grad(near) or _requires_grad(far)))
        in_req = grad_enabled and (_requires_grad(rays_o) or _requires_grad(rays_d) or z_req or
                                   (mvps and _requires_grad(lights_dir)) or (not mvps and _requires_grad(background_rgb)))
        if in_req and (self.desc.variant & native.VARIANT_BF16):
            raise RuntimeError("NeuSRenderer: gradients with respect to rays, lights, background or z are not available "
                               "with set_variant(bf16=True) (the bf16 sweeps have no input adjoints); use the default "
                               "variant, or detach those inputs")
        # (differentiable: a float32 contiguous input is passed through as is, with its bits)
        rays_o = rays_o.to(torch.float32).contiguous()
        rays_d = rays_d.to(torch.float32).contiguous()
        packed = self._pack(use_color)
        perturb = self.perturb if perturb_overwrite < 0 else perturb_overwrite
        if z_vals is None:
            with torch.no_grad():
                z_vals = self.sample_z_vals(rays_o.detach(), rays_d.detach(), near, far, packed, perturb, t_rand)
            if z_req and grad_enabled:
                z_vals = _ZFromNearFar.apply(near, far, z_vals)
        else:
            z_vals = z_vals.to(torch.float32).contiguous()
        self.last_z_vals = z_vals.detach()
        lights = None
        if mvps:
            L = lights_dir.shape[0]
            lt = lights_dir.to(torch.float32)
            if lt.numel() == L * 3:
                lights = lt.reshape(L, 3).contiguous()
            else:
                lights = lt.reshape(L, B, 3).contiguous()
                flags |= native.FLAG_LIGHT_PER_RAY
        bg = None
        if background_rgb is not None and not mvps:
            bg = background_rgb.to(torch.float32).reshape(3).contiguous()
        # leaves that receive gradients: as in exp_runner.py:105-112 the albedo net is trained unless no_albedo
        train_color = use_color
        leaves = self._leaves(train_color)
        grad_on = grad_enabled and (in_req or any(p.requires_grad for p in leaves))
        if not grad_on:
            flags |= native.FLAG_FORWARD_ONLY
        if in_req:
            flags |= native.FLAG_INPUT_GRADS
        call = dict(rays_o=rays_o, rays_d=rays_d, z_vals=z_vals, lights=lights, background_rgb=bg,
                    cos_anneal_ratio=cos_anneal_ratio, flags=flags, packed=packed, leaves=leaves,
                    train_color=train_color, want_extras=self.want_extras)
        outs = _FinePass.apply(self, call, rays_o, rays_d, lights, bg, z_vals, *leaves)
        out = dict(zip(_OUT_KEYS, outs))
        token = getattr(self, "_last_dp_token", None)
        self._last_dp_token = None
        if token is not None:
            out["gradient_error"].rnb_dp_token = token
        return out

    # ------------------------------------------------------------------ reference API
    def render(self, rays_o, rays_d, near, far, perturb_overwrite=-1, background_rgb=None, cos_anneal_ratio=0.0,
               t_rand=None, z_vals=None):
        """models/renderer.py:556-648."""
        return self._run(rays_o, rays_d, near, far, None, perturb_overwrite, background_rgb, cos_anneal_ratio,
                         native.MODE_CORE, t_rand, z_vals)

    def render_rnb_warmup(self, rays_o, rays_d, near, far, lights_dir, perturb_overwrite=-1, background_rgb=None,
                          cos_anneal_ratio=0.0, no_albedo=False, t_rand=None, z_vals=None):
        """models/renderer.py:828-930 (ReLU on the shading)."""
        flags = native.MODE_MVPS | native.FLAG_RELU_SHADING | (native.FLAG_NO_ALBEDO if no_albedo else 0)
        return self._run(rays_o, rays_d, near, far, lights_dir, perturb_overwrite, background_rgb, cos_anneal_ratio,
                         flags, t_rand, z_vals)

    def render_rnb(self, rays_o, rays_d, near, far, lights_dir, perturb_overwrite=-1, background_rgb=None,
                   cos_anneal_ratio=0.0, no_albedo=False, t_rand=None, z_vals=None):
        """models/renderer.py:932-1033."""
        flags = native.MODE_MVPS | (native.FLAG_NO_ALBEDO if no_albedo else 0)
        return self._run(rays_o, rays_d, near, far, lights_dir, perturb_overwrite, background_rgb, cos_anneal_ratio,
                         flags, t_rand, z_vals)

    # ------------------------------------------------------------------ whole images (forward only)
    def _maps_begin(self, n_rays, S, api, no_albedo, maps, n_lights, chunk_rays, background_rgb, cos_anneal_ratio, dev,
                    keep_z):
        """Everything the chunks of one whole-image render share: flags, packed weights, the preallocated outputs and
        ONE workspace of the one-chunk size."""
        if api not in _MAPS_API:
            raise ValueError(f"render_maps: unknown api {api!r} (one of {sorted(_MAPS_API)})")
        if self.sdf_network.lin0.bias.device != dev:
            raise RuntimeError(f"NeuSRenderer: rays live on {dev} but the networks on "
                               f"{self.sdf_network.lin0.bias.device}")
        flags = _MAPS_API[api]
        mvps = bool(flags & native.MODE_MVPS)
        if mvps and no_albedo:
            flags |= native.FLAG_NO_ALBEDO
        use_color = not (mvps and no_albedo)
        has_albedo = mvps and use_color
        if maps is DEFAULT_MAPS:          # the default set: every map this mode has
            maps = tuple(m for m in maps if m != "albedo" or has_albedo)
        maps = tuple(maps)
        unknown = [m for m in maps if m not in _MAPS_KNOWN]
        if unknown or not maps:
            raise ValueError(f"render_maps: maps must be a non-empty subset of {_MAPS_KNOWN}, not {maps}")
        if "albedo" in maps and not has_albedo:
            raise ValueError("render_maps: the albedo map exists for render_rnb / render_rnb_warmup with the albedo network "
                             "only (not api='render', not no_albedo=True)")
        # (a larger S than kMaxS is refused by the workspace query below; the light count only by the call itself, which
        # without explicit depths would come after the sampler's launches)
        if mvps and n_lights > native.MAX_RENDER_LIGHTS:
            raise ValueError(f"render_maps: n_lights {n_lights} > {native.MAX_RENDER_LIGHTS} (kMaxRenderLights)")
        chunk = max(1, min(int(chunk_rays), n_rays))
        Cd = self.desc.col_d_out
        f32 = dict(dtype=torch.float32, device=dev)
        shapes = {"color": (n_lights, n_rays, Cd) if mvps else (n_rays, 3), "normal": (n_rays, 3), "albedo": (n_rays, Cd),
                  "depth": (n_rays, 1), "weight_sum": (n_rays, 1), "weight_max": (n_rays, 1)}
        out = {m: torch.empty(shapes[m], **f32) for m in maps}
        if keep_z:
            out["z_vals"] = torch.empty(n_rays, S, **f32)
        ws_bytes = native.workspace_bytes("render", C.byref(self.desc), chunk, S, flags | native.FLAG_FORWARD_ONLY, floor=256)
        bg = None
        if background_rgb is not None and not mvps:
            bg = background_rgb.detach().to(device=dev, dtype=torch.float32).reshape(3).contiguous()
        return dict(flags=flags, mvps=mvps, maps=maps, out=out, chunk=chunk, S=S, L=n_lights, Cd=Cd, dev=dev, bg=bg,
                    packed=self._pack(use_color), ws=torch.empty(ws_bytes, dtype=torch.uint8, device=dev),
                    cos=float(cos_anneal_ratio), variance=self.deviation_network.variance.detach().reshape(1))

    def _maps_chunk(self, st, i0, rays_o, rays_d, z_vals, lights):
        """One chunk of a whole-image render into rows [i0, i0 + n) of the outputs; the workspace is the shared one (stream
        order makes the reuse safe: every chunk's kernels are enqueued behind the previous chunk's)."""
        n = rays_o.shape[0]
        out, flags = st["out"], st["flags"]
        args = native.RenderArgs()
        args.B, args.S, args.n_lights, args.flags = n, st["S"], st["L"] if st["mvps"] else 1, flags
        args.cos_anneal_ratio = st["cos"]
        args.rays_o, args.rays_d, args.z_vals = rays_o.data_ptr(), rays_d.data_ptr(), z_vals.data_ptr()
        args.variance = st["variance"].data_ptr()
        args.background_rgb = st["bg"].data_ptr() if st["bg"] is not None else None
        if st["mvps"]:
            if lights.numel() != st["L"] * 3:
                args.flags |= native.FLAG_LIGHT_PER_RAY
            args.lights_dir = lights.data_ptr()
        m = native.RenderMapsOut()
        block = None
        for k in st["maps"]:
            if k == "color" and st["mvps"]:
                if n == out[k].shape[1]:
                    m.color = out[k].data_ptr()
                else:   # [L,B,C] colour: the kernel writes the chunk's contiguous [L,n,C] block, copied into its columns below
                    block = torch.empty(st["L"], n, st["Cd"], dtype=torch.float32, device=st["dev"])
                    m.color = block.data_ptr()
            else:
                setattr(m, k, out[k][i0:i0 + n].data_ptr())
        native.same_device(st["packed"], rays_o, rays_d, z_vals, lights, st["ws"])
        with native.on_device(st["dev"]) as stream:
            native.check(native.load().rnb_render_maps(C.byref(self.desc), native.ptr(st["packed"]), C.byref(args),
                                                       C.byref(m), native.ptr(st["ws"]), st["ws"].numel(), stream))
        if block is not None:
            out["color"][:, i0:i0 + n].copy_(block)
        if "z_vals" in out:
            out["z_vals"][i0:i0 + n].copy_(z_vals)

    @staticmethod
    def _maps_lights(lights_dir, n_rays, dev):
        if lights_dir is None:
            raise ValueError("render_maps: render_rnb / render_rnb_warmup need lights_dir")
        L = lights_dir.shape[0]
        lt = lights_dir.detach().to(device=dev, dtype=torch.float32)
        if lt.numel() == L * 3:
            return lt.reshape(L, 3).contiguous(), False
        return lt.reshape(L, n_rays, 3), True

    @torch.no_grad()
    def render_maps(self, rays_o, rays_d, near, far, lights_dir=None, *, api="render_rnb", perturb_overwrite=-1,
                    background_rgb=None, cos_anneal_ratio=0.0, no_albedo=False, t_rand=None, z_vals=None,
                    chunk_rays=DEFAULT_CHUNK_RAYS, maps=DEFAULT_MAPS, return_z_vals=False):
        """Forward-only render of ANY number of rays to per-ray maps (`rnb_render_maps`): what `validate_image`
        (exp_runner.py:460-470) reduces from the training dictionary with torch ops and a `.cpu()` per batch.  `api` names
        the wrapper whose arithmetic is wanted ("render", "render_rnb", "render_rnb_warmup"); the other arguments are that
        wrapper's.  Returns a dict with the requested `maps`:
          color [L,B,C] (render: [B,3], background included) — `color_fine` of the wrapper, bit for bit when one chunk
          holds the same rays; normal [B,3] = sum_s w n [|p| < 1]; albedo [B,C] = sum_s w albedo (render_rnb* with the
          albedo network only; the default `maps` leaves it out where it does not exist, asking for it there raises);
          depth [B,1] = sum_s w (z + dists / 2); weight_sum, weight_max [B,1]; z_vals [B,S] with `return_z_vals`.
        The rays run in chunks of `chunk_rays` through ONE workspace of the one-chunk size, allocated once (stream order
        makes the reuse safe), and every chunk's maps are written straight into rows of the preallocated outputs — except
        [L,B,C] colour, whose per-chunk [L,n,C] block is copied into its columns (the kernel has no output stride).
        Workspace: `rnb_render_workspace_bytes` of (desc, chunk_rays, S, flags | RNB_FLAG_FORWARD_ONLY) — about 30 KB per
        sample point at the shipped shape (256-wide, 8 layers), i.e. ~4 GB per 1024-ray chunk of 128 samples, whatever the
        image size.  Runs under no_grad whatever the caller's grad mode (outputs carry no grad_fn, no `.grad` is touched),
        for every `set_variant`, and is never collective under `set_data_parallel`."""
        if not rays_o.is_cuda:
            raise RuntimeError("NeuSRenderer: rays must be on the GPU (no CPU path; librnbneus_hip.so only)")
        dev = rays_o.device
        N = rays_o.shape[0]
        rays_o = rays_o.detach().to(torch.float32).contiguous()
        rays_d = rays_d.detach().to(torch.float32).contiguous()
        mvps = bool(_MAPS_API.get(api, 0) & native.MODE_MVPS)
        lights, per_ray = self._maps_lights(lights_dir, N, dev) if mvps else (None, False)
        if z_vals is not None:
            z_vals = z_vals.detach().to(torch.float32).contiguous()
        S = z_vals.shape[1] if z_vals is not None else self.n_samples + self.n_importance
        st = self._maps_begin(N, S, api, no_albedo, maps, lights.shape[0] if mvps else 1, chunk_rays, background_rgb,
                              cos_anneal_ratio, dev, return_z_vals)
        perturb = self.perturb if perturb_overwrite < 0 else perturb_overwrite
        near = near.detach().reshape(N)
        far = far.detach().reshape(N)
        if t_rand is not None:
            t_rand = t_rand.detach().reshape(N, 1)
        for i0 in range(0, N, st["chunk"]):
            i1 = min(N, i0 + st["chunk"])
            o, d = rays_o[i0:i1], rays_d[i0:i1]
            if z_vals is None:
                z = self.sample_z_vals(o, d, near[i0:i1], far[i0:i1], st["packed"], perturb,
                                       None if t_rand is None else t_rand[i0:i1])
            else:
                z = z_vals[i0:i1]
            self._maps_chunk(st, i0, o, d, z, lights[:, i0:i1].contiguous() if per_ray else lights)
        return st["out"]

    @torch.no_grad()
    def render_image(self, rays, img_idx=None, *, pose=None, light=None, resolution_level=1, warmup=False, api=None,
                     perturb_overwrite=-1, background_rgb=None, cos_anneal_ratio=0.0, no_albedo=False,
                     chunk_rays=DEFAULT_CHUNK_RAYS, maps=DEFAULT_MAPS, return_z_vals=False, to_host=False):
        """One whole view as images, everything on the device (`validate_image` / `render_novel_image`,
        exp_runner.py:389-558): per chunk of `chunk_rays` rays, `rays.view_rays` (rays, near / far, the lights at the
        rounded pixel: one launch), the sampler and `rnb_render_maps` into rows of the preallocated images.
        `rays`: a `DeviceRays`; `img_idx` a view of it, or `pose` [4,4] for a novel view (`rays.pose_between`; no lights:
        api="render").  `light`: one light index or None for all (Lo = 1 or n_lights); `warmup`: the warm-up lights and
        images.  `api` defaults to "render_rnb_warmup" with `warmup`, "render" for a pose-only view, else "render_rnb".
        Returns `color` [Lo,Hl,Wl,C] (render: [Hl,Wl,3]), `normal` [Hl,Wl,3], `albedo` [Hl,Wl,C], `depth`, `weight_sum`,
        `weight_max` [Hl,Wl] (those asked for in `maps`), `mask` [Hl,Wl] and `true_rgb` [Lo,Hl,Wl,3] (None for a pose-only
        view) and with `return_z_vals` `z_vals` [Hl*Wl,S].  No host synchronisation, unless `to_host=True` asks for numpy
        copies: then exactly one, after the last chunk.  The other keywords are `render_maps`'."""
        gather = img_idx is not None
        if api is None:
            api = "render_rnb_warmup" if warmup else ("render_rnb" if gather else "render")
        mvps = bool(_MAPS_API.get(api, 0) & native.MODE_MVPS)
        dev = rays.device
        tx, ty = rays._grid(resolution_level)[:2]
        Hl, Wl = ty.numel(), tx.numel()
        N = Hl * Wl
        if mvps and (not gather or not rays.has_lights(warmup)):
            raise ValueError(f"render_image: api={api!r} needs the lights of a view (img_idx), or api='render'")
        n_rgb = rays.n_lights if light is None else 1
        Lo = n_rgb if mvps else 1
        S = self.n_samples + self.n_importance
        st = self._maps_begin(N, S, api, no_albedo, maps, Lo, chunk_rays, background_rgb, cos_anneal_ratio, dev,
                              return_z_vals)
        perturb = self.perturb if perturb_overwrite < 0 else perturb_overwrite
        f32 = dict(dtype=torch.float32, device=dev)
        mask = torch.empty(N, 1, **f32) if gather else None
        true_rgb = torch.empty(n_rgb, N, 3, **f32) if gather else None
        for i0 in range(0, N, st["chunk"]):
            n = min(N, i0 + st["chunk"]) - i0
            r = rays.view_rays(img_idx, pose, resolution_level, light, warmup, i0, n)
            o, d = r["rays_o"].contiguous(), r["rays_d"].contiguous()
            z = self.sample_z_vals(o, d, r["near"], r["far"], st["packed"], perturb)
            lights = None
            if mvps:
                lights, _ = self._maps_lights(r["lights_dir"], n, dev)
                lights = lights.contiguous()
            self._maps_chunk(st, i0, o, d, z, lights)
            if gather:
                mask[i0:i0 + n].copy_(r["mask"])
                true_rgb[:, i0:i0 + n].copy_(r["true_rgb"])
        img = {}
        for k, v in st["out"].items():
            if k == "color":
                img[k] = v.reshape(Lo, Hl, Wl, -1) if mvps else v.reshape(Hl, Wl, 3)
            elif k == "z_vals":
                img[k] = v
            else:
                img[k] = v.reshape(Hl, Wl, -1) if k in ("normal", "albedo") else v.reshape(Hl, Wl)
        img["mask"] = mask.reshape(Hl, Wl) if gather else None
        img["true_rgb"] = true_rgb.reshape(-1, Hl, Wl, 3) if gather else None
        if to_host:
            host = {k: (None if v is None else torch.empty(v.shape, dtype=v.dtype, pin_memory=True).copy_(v, non_blocking=True))
                    for k, v in img.items()}
            torch.cuda.current_stream(dev).synchronize()    # the one synchronisation of a whole image
            img = {k: (None if v is None else v.numpy()) for k, v in host.items()}
        return img

    def color(self, points, normals, view_dirs, feature_vectors):
        """RenderingNetwork.forward through this renderer's packed weights (view_dirs unused in
        no_view_dir mode, models/fields.py:190-192)."""
        packed = self._pack(True)
        return runtime.color_forward(self.desc, packed, points, normals, feature_vectors)

    def extract_fields(self, bound_min, bound_max, resolution, chunk=64, group=None, to_host=True):
        """SDF grid query of models/renderer.py:10-25 (values negated as at :1224): `resolution`^3 forward-only
        evaluations.  The grid points are generated inside the forward kernel (`rnb_sdf_grid`), the volume is
        assembled on the device and copied to the host once (`to_host=False` returns the device tensor).  With data
        parallelism enabled (`set_data_parallel`) or a `group` given, every rank evaluates one contiguous x-slab and
        the slabs are exchanged with one all-gather (512^3: 512 MB in total).  `chunk` is accepted for signature
        compatibility with the reference's block size N = 64 and has no effect: every point is evaluated once,
        whatever the blocking."""
        dev = self.sdf_network.lin0.bias.device
        packed = self._pack(False)
        lib = native.load()
        res = int(resolution)
        group = group if group is not None else self.dp_group
        rank, world = (dist.get_rank(group), dist.get_world_size(group)) if group is not None else (0, 1)
        per, x0, x1 = parallel.grid_slab(res, rank, world)   # x-planes per rank (the last slabs may be shorter, or empty)
        gd = mesh_pipeline.grid_desc(bound_min, bound_max, res, x0, x1)
        slab = torch.empty(per, res, res, dtype=torch.float32, device=dev)     # padded to `per` planes for the gather
        with torch.no_grad():
            if x1 > x0:
                ws = native.workspace("sdf_grid", dev, C.byref(self.desc), C.byref(gd), floor=256)
                with native.on_device(dev) as stream:
                    native.check(lib.rnb_sdf_grid(C.byref(self.desc), native.ptr(packed), C.byref(gd), native.ptr(slab),
                                                  native.ptr(ws), ws.numel(), stream))
            if x1 - x0 < per:
                slab[x1 - x0:].zero_()
            if world > 1:
                u = parallel.gather_grid_slabs(slab, res, group)
            else:
                u = slab[:res]
        return u.cpu().numpy() if to_host else u

    def extract_fields_sparse(self, bound_min, bound_max, resolution, threshold=0.0, brick=None, margin=1.0, to_host=False):
        """The volume of `extract_fields` with only the bricks near the iso-surface evaluated (`rnb_sdf_grid_sparse_*`,
        include/rnbneus.h has the contract).  Returns `(u, info)`: `u` [res,res,res] — samples of the evaluated bricks are
        bit-equal to `extract_fields`', every other sample holds the clamped trilinear interpolant of its brick's corner
        values, which lies on the corners' side of `threshold` — so marching cubes at `threshold` gives the dense volume's
        mesh for every surface component that passes through a seed brick.  `brick`: cells per brick edge (4, 8, 16, 32;
        None = `DEFAULT_SPARSE_BRICK`); `margin`: the Lipschitz constant of the SDF to assume when seeding (1.0 is exact
        for a true distance field; 0 seeds from sign changes between brick corners only; a component lying wholly inside
        bricks whose corners are farther than margin x half a brick diagonal from the threshold is missed).
        `info`: `brick`, `bricks_total`, `bricks_seeded`, `bricks_active`, `rounds` (growth rounds that listed new
        bricks), `points_evaluated` (brick-corner lattice + (brick+1)^3 per evaluated brick) and `mask` (bool [nb,nb,nb]
        device tensor of the evaluated bricks).  The host reads one 8-byte counter per round.  Data-parallel sparse grids
        do not exist: with `set_data_parallel` enabled this raises rather than run replicated."""
        res = int(resolution)
        brick = DEFAULT_SPARSE_BRICK if brick is None else int(brick)
        geo = native.brick_geometry(res, brick)   # (ValueError for a resolution below 2 or an unknown brick size)
        margin, threshold = float(margin), float(threshold)
        if not margin >= 0.0:
            raise ValueError(f"extract_fields_sparse: margin must be >= 0, not {margin}")
        if threshold != threshold:
            raise ValueError("extract_fields_sparse: threshold is NaN")
        if geo["bricks_total"] > 2 ** 31 - 1:
            raise ValueError(f"extract_fields_sparse: {geo['bricks_total']} bricks do not fit a 32-bit id")
        if self.dp_group is not None:
            raise ValueError("extract_fields_sparse: data-parallel sparse grids are not supported "
                             "(extract_fields serves set_data_parallel)")
        dev = self.sdf_network.lin0.bias.device
        if dev.type != "cuda":
            raise RuntimeError(native.NO_CPU_PATH)
        lib = native.load()
        gd = mesh_pipeline.grid_desc(bound_min, bound_max, res, 0, res)
        sd = native.SparseGridDesc(brick, threshold, margin)
        nb = geo["nb"]
        with torch.no_grad():
            packed = self._pack(False)
            ws = native.workspace("sdf_grid_sparse", dev, C.byref(self.desc), C.byref(gd), C.byref(sd), floor=256)
            u = torch.empty(res, res, res, dtype=torch.float32, device=dev)
            mask = torch.empty(nb, nb, nb, dtype=torch.uint8, device=dev)
            n_listed = torch.zeros(1, dtype=torch.int64, device=dev)
            with native.on_device(dev) as stream:
                native.check(lib.rnb_sdf_grid_sparse_seed(C.byref(self.desc), native.ptr(packed), C.byref(gd), C.byref(sd),
                                                          native.ptr(ws), ws.numel(), native.ptr(n_listed), stream))
                seeded = n = int(n_listed.item())
                first, rounds = 0, 0
                while first < n:   # evaluate the list's tail, grow from it; every launch is sized from a count read here
                    native.check(lib.rnb_sdf_grid_sparse_round(C.byref(self.desc), native.ptr(packed), C.byref(gd),
                                                               C.byref(sd), native.ptr(u), native.ptr(ws), ws.numel(), first,
                                                               n - first, native.ptr(n_listed), stream))
                    first, n = n, int(n_listed.item())
                    rounds += 1 if n > first else 0
                native.check(lib.rnb_sdf_grid_sparse_finish(C.byref(self.desc), C.byref(gd), C.byref(sd), native.ptr(u),
                                                            native.ptr(ws), ws.numel(), native.ptr(mask), stream))
        info = {"brick": brick, "bricks_total": geo["bricks_total"], "bricks_seeded": seeded, "bricks_active": n,
                "rounds": rounds, "points_evaluated": (nb + 1) ** 3 + n * geo["samples"] ** 3, "mask": mask.bool()}
        return (u.cpu().numpy() if to_host else u), info

    def _collect_range(self, desc, packed, ws, B, S, flags):
        if self._range is None or self._range.device != ws.device:
            self._range = torch.zeros(8, dtype=torch.float32, device=ws.device)
        with native.on_device(ws.device) as stream:
            native.check(native.load().rnb_render_range(C.byref(desc), native.ptr(packed), native.ptr(ws), ws.numel(), B, S,
                                                        flags, native.ptr(self._range), stream))

    def range_report(self):
        """Largest operand magnitudes of the last render made with `track_range = True` (one device-to-host copy):
        `max_abs_weight`, `max_abs_activation` (SDF network, incl. the encoded input), `max_abs_jacobian_row`,
        `max_abs_albedo_activation`, `max_abs_adjoint` (after a backward; 0 for forward-only renders), `dead_tiles` (64-point
        tiles whose colour adjoint was exactly zero and which the backward skipped; 0 where it skips none).  The default arithmetic
        takes every operand scale from the data (include/rnbneus.h, RNB_VARIANT_X2H): none of these has a limit; the
        numbers say how far a model is from the range the fixed scales of ABI 4 assumed (weights 255, activations 1023)."""
        if self._range is None:
            raise RuntimeError("range_report(): set `track_range = True` and render first")
        r = [float(x) for x in self._range.cpu()]
        return {"max_abs_weight": r[0], "max_abs_activation": r[1], "max_abs_jacobian_row": r[2],
                "max_abs_albedo_activation": r[3], "max_abs_adjoint": r[4], "dead_tiles": int(r[5])}

    def x2h_range_report(self):
        """Host-side (plain torch) maximum of |g v / ||v||| over every layer of both networks:
        `{"max_abs_weight": m, "layer": name, "limit": 255.0, "ok": m < 255}`.  Kept from ABI 4, where a weight beyond 255
        overflowed the fixed fp16 scale of the default arithmetic; since ABI 5 the scale of every matrix is taken from its own
        maximum and `ok` is informative only.  `range_report()` gives the device-side maxima of a whole render."""
        worst, where = 0.0, None
        with torch.no_grad():
            for prefix, net in (("sdf", self.sdf_network), ("color", self.color_network)):
                for i, lin in enumerate(net.lins()):
                    if hasattr(lin, "weight_g"):
                        v = lin.weight_v.detach().double()
                        w = lin.weight_g.detach().double().reshape(-1, 1) * v / v.norm(dim=1, keepdim=True)
                    else:
                        w = lin.weight.detach().double()
                    m = float(w.abs().max())
                    if m > worst or where is None:
                        worst, where = m, f"{prefix}.lin{i}"
        return {"max_abs_weight": worst, "layer": where, "limit": 255.0, "ok": bool(worst < 255.0)}

    def extract_geometry(self, bound_min, bound_max, resolution, threshold=0.0, backend=None, sparse=False, margin=1.0,
                         brick=None, clean=None, simplify=None, cull=None, fill=None):
        """models/renderer.py:1219-1224 / :27-36: SDF grid + marching cubes + rescaling to the bounding box; returns
        numpy `(vertices [V,3] float64, triangles [T,3])` as the reference does.
        `backend`: "native" — the library's own marching cubes on the volume still resident in HBM
        (csrc/mcubes.hip); "mcubes" — PyMCubes on the host copy, exactly the reference's call (raises ImportError when
        PyMCubes is not installed); None (default) — "mcubes" when it is importable (the reference-faithful default),
        else "native".  The choice made for None is logged once per process (logger `rnb_neus_fork_amd`, INFO) and kept in
        `self.last_mesh_backend`, so the same script cannot silently produce different triangulations on two machines.
        The native mesh has the same vertices (one per crossed grid edge, same interpolation); its triangulation of
        ambiguous cells / quad diagonals may differ from PyMCubes' table (parity unpinned: DESIGN).
        `sparse=True`: the volume comes from `extract_fields_sparse(threshold=threshold, margin=margin, brick=brick)` —
        only the bricks near the surface are evaluated, the mesh is the dense one for every component that passes through
        a seed brick (see there for what `margin` can miss) — and its `info` is kept in `self.last_sparse_grid`.  Marching
        cubes itself is unchanged and runs over the dense array; its limit of 2^32 grid points caps `resolution` at 1625
        either way.
        `clean`: a dict of `mesh_clean.clean_mesh` keywords, e.g. `{"keep_largest": 1}` — the mesh is cleaned on the device
        before the rescaling (areas are measured in grid-index units; with `backend="mcubes"` the host arrays are uploaded
        for it) and the `info` of the cleaning is kept in `self.last_mesh_clean`.  None (default): no cleaning.
        `simplify`: a dict of `mesh_simplify.simplify_mesh` keywords (`cell_size` in grid-index units, i.e. voxels, or
        `target_triangles`; `origin`) — the mesh is simplified on the device after the cleaning and before the rescaling;
        `info` is kept in `self.last_mesh_simplify`.  None (default): no simplification.
        `cull`: a dict of `mesh_cull.cull_mesh` keywords (`rays` or `projections` / `eyes` / `masks` / `image_size`; `views`,
        `max_outside`, `min_seen`, `occlusion`, `dilate`, `threshold`, `rule`) — what the cameras do not support is removed
        on the device after the cleaning and before the simplification; the votes are taken on the vertices rescaled to the
        bounding box (the cameras' frame), `info` is kept in `self.last_mesh_cull`.  None (default): no culling.
        `fill`: a dict of `mesh_fill.fill_holes` keywords (`max_edges`; `{}` fills every simple loop) — the holes the mesh has
        after the stages are closed with centroid fans on the device, last before the rescaling; `info` is kept in
        `self.last_mesh_fill`.  None (default): no filling."""
        if backend is None:
            try:
                import mcubes  # noqa: F401
                backend = "mcubes"
            except ImportError:
                backend = "native"
            global _MESH_BACKEND_LOGGED
            if not _MESH_BACKEND_LOGGED:
                _MESH_BACKEND_LOGGED = True
                logging.getLogger("rnb_neus_fork_amd").info(
                    "extract_geometry(backend=None): using %r (%s); pass backend= to fix the choice", backend,
                    "PyMCubes is importable" if backend == "mcubes" else "PyMCubes is not installed")
        self.last_mesh_backend = backend
        if backend not in ("native", "mcubes"):
            raise ValueError(f"extract_geometry: unknown backend {backend!r}")
        options = {"clean": clean, "simplify": simplify, "cull": cull}
        mesh_pipeline.check_options(**options, fill=fill)
        if backend == "mcubes":
            import mcubes
            u = mesh_pipeline.volume(self, bound_min, bound_max, resolution, threshold, sparse, brick, margin, to_host=True)
            vertices, triangles = mcubes.marching_cubes(u, threshold)
            if fill is not None or any(o is not None for o in options.values()):     # the stages run on the device: the host arrays go up for them
                dev = self.sdf_network.lin0.bias.device
                v = torch.as_tensor(np.ascontiguousarray(vertices, dtype=np.float64)).to(dev)
                t = torch.as_tensor(np.ascontiguousarray(triangles).astype(np.int32)).to(dev)
                v, t = mesh_pipeline.run_stages(self, v, t, (bound_min, bound_max, resolution), options)
                v, t = mesh_pipeline.run_fill(self, v, t, fill)
                vertices, triangles = v.cpu().numpy(), t.cpu().numpy()
        else:
            v, t = mesh_pipeline.device_mesh(self, bound_min, bound_max, resolution, threshold, sparse, brick, margin, options,
                                             fill)
            vertices, triangles = v.cpu().numpy(), t.cpu().numpy()
        return mesh_pipeline.rescale_to_bounds_host(vertices, bound_min, bound_max, resolution), triangles

    # ------------------------------------------------------------------ textured mesh (validate_mesh_texture)
    @torch.no_grad()
    def vertex_attributes(self, points=None, *, grid_vertices=None, bounds=None, resolution=None, threshold=0.0, refine=0,
                          max_step=None, albedo=None, chunk=65536):
        """Per-vertex attributes on the device (`rnb_mesh_vertex_attrs`): what `validate_mesh_texture`
        (exp_runner.py:601-613) gets from `sdf_network(v)`, `sdf_network.gradient(v)` and `color_network(v, g, g, feat)` per
        host chunk — one forward, one reverse and one albedo sweep per chunk of `chunk` vertices on the model's kernel
        route, through one workspace of the one-chunk size.
        Vertices: fp32 model-space `points` [V,3], or float64 `grid_vertices` [V,3] as `marching_cubes` returns them with
        `bounds` = (bound_min, bound_max) and `resolution` (rescaled on the device, bit for bit `extract_geometry`'s
        expression converted to float32).  `refine` Newton steps move every vertex towards sdf = -threshold, each by at
        most `max_step` (default with grid vertices: one cell diagonal; bare points must state it).
        Returns device tensors `points` [V,3] (where the attributes were evaluated), `sdf` [V,1], `gradient` [V,3]
        (unnormalised, the albedo net's normal input), `normal` [V,3] (unit, or 0) and, with the albedo network, `albedo`
        [V,col_d_out] and `rgb` [V,3] uint8 = rint(255 clip(albedo[:, [2,1,0]], 0, 1)).  `albedo=None`: if the renderer has
        the network.  Runs under no_grad whatever the caller's grad mode and is never collective under
        `set_data_parallel`."""
        if (points is None) == (grid_vertices is None):
            raise ValueError("vertex_attributes: give either points or grid_vertices")
        has_albedo = self.color_network is not None
        albedo = has_albedo if albedo is None else bool(albedo)
        if albedo and not has_albedo:
            raise ValueError("vertex_attributes: albedo=True on a renderer without an albedo network")
        refine = int(refine)
        if refine < 0:
            raise ValueError(f"vertex_attributes: refine must be >= 0, not {refine}")
        lo = hi = None
        if grid_vertices is not None:
            if bounds is None or resolution is None:
                raise ValueError("vertex_attributes: grid_vertices need bounds=(bound_min, bound_max) and resolution")
            resolution = int(resolution)
            if resolution < 2:
                raise ValueError(f"vertex_attributes: a grid of resolution {resolution} has no cells")
            lo, hi = ([float(b[d]) for d in range(3)] for b in bounds)
            if max_step is None:
                max_step = mesh_pipeline.cell_diagonal(lo, hi, resolution)
        if refine > 0 and (max_step is None or not float(max_step) > 0.0):
            raise ValueError("vertex_attributes: refine > 0 needs max_step > 0 (bare points have no cell size to default to)")
        src = grid_vertices if grid_vertices is not None else points
        dev = self.sdf_network.lin0.bias.device
        if dev.type != "cuda":
            raise RuntimeError(native.NO_CPU_PATH)
        if src.device != dev:
            raise RuntimeError(f"NeuSRenderer: vertices live on {src.device} but the networks on {dev}")
        return runtime.mesh_vertex_attrs(self.desc, self._pack(albedo), points=points, grid_vertices=grid_vertices,
                                         bound_min=lo, bound_max=hi, resolution=resolution or 0, level=-float(threshold),
                                         refine=refine, max_step=float(max_step) if max_step is not None else 0.0,
                                         albedo=albedo, swap_rb=True, chunk=chunk)

    @torch.no_grad()
    def bake_textures(self, vertices, triangles, *, size=None, chart=None, refine=0, max_step=None, threshold=0.0,
                      albedo=None, slab=1 << 20, chunk=65536, return_samples=False, to_host=True):
        """Bakes the field into textures of a mesh, on the device (texture_bake.py; include/rnbneus.h "Texture baking").
        vertices [V,3] float64 in MODEL space and triangles [T,3] int32, device tensors as
        `extract_textured_geometry(to_host=False)` returns them.  Every triangle gets a chart of `chart` texel steps
        (`texture_bake.atlas_layout(T, size, chart)`: `chart` alone sizes the image, `size` alone takes the largest chart
        that fits size x size, neither: chart = 8) with (chart + 1)(chart + 2) / 2 lattice samples; per slab of `slab`
        samples (a positive multiple of 64, so the 64-point tiles of the sweeps — and their per-tile scales — are the same
        whatever the slab) `rnb_texture_sample_points` makes the fp32 points and `vertex_attributes(points, refine=,
        max_step=, threshold=, chunk=)` evaluates them; one `rnb_texture_pack` writes the images.  `refine` > 0 (needs
        `max_step`, model-space units) projects every sample onto the level set first, so the maps carry the detail the
        simplification removed.  Returns a dict: `uv` [T,3,2] float64 (per corner; v up), `albedo_image` [H,W,4] uint8
        (RGB of the per-vertex colour rule, alpha 255, empty texels 0; None without the albedo network: `albedo=None` means
        "if the renderer has it", `albedo=True` raises without it), `normal_image` [H,W,4] uint8 (object-space unit normals
        in model space, rint(255 (0.5 n + 0.5))), `texel_sample` [H,W] int32 (the sample of every texel, -1 where empty:
        the gather map for float channels), `layout` (`AtlasLayout`), `info` (`samples`, `bad_triangles`: triangles with
        an index outside [0, V) or a non-finite corner, whose texels are empty; `slabs`) and, with `return_samples`, the
        per-sample `points` [N,3], `sdf` [N,1], `normal` [N,3] and `albedo` [N,C] float32.  numpy arrays, or device
        tensors with `to_host=False`.  Runs under no_grad; one host read (the bad-triangle counter); never collective
        under `set_data_parallel`."""
        from .texture_bake import bake_textures
        return bake_textures(self, vertices, triangles, size=size, chart=chart, refine=refine, max_step=max_step,
                             threshold=threshold, albedo=albedo, slab=slab, chunk=chunk, return_samples=return_samples,
                             to_host=to_host)

    @torch.no_grad()
    def extract_textured_geometry(self, bound_min, bound_max, resolution, threshold=0.0, *, sparse=False, margin=1.0,
                                  brick=None, refine=0, max_step=None, chunk=65536, to_host=True, clean=None,
                                  simplify=None, bake=None, cull=None, fill=None):
        """`validate_mesh_texture` up to the export (exp_runner.py:584-613): SDF grid (dense, or `sparse=True` as in
        `extract_geometry`), the native marching cubes, and `vertex_attributes` on the vertices where marching cubes left
        them — they never leave the device in between.  Returns a dict:
          `vertices` [V,3] float64 rescaled to the bounding box and `triangles` [T,3] int32 — with `refine == 0` the arrays
          of `extract_geometry(..., backend="native")`; with `refine > 0` the float64 of the refined fp32 points (each moved
          by at most `max_step`, default one cell diagonal, per step);
          `normals` [V,3] float32 (unit); `sdf` [V,1]; and with the albedo network `albedo` [V,col_d_out] and `colors` [V,3]
          uint8 RGB, the reference's `clip(albedo[:, [2,1,0]], 0, 1)` quantised by rint(255 x).
        numpy arrays, or device tensors with `to_host=False` (then the only host synchronisations after the SDF grid are
        the two marching-cubes counts).  `mesh_io.write_ply` writes the result.
        `clean`: a dict of `mesh_clean.clean_mesh` keywords, e.g. `{"keep_largest": 1}`; the cleaning runs between marching
        cubes and `vertex_attributes`, so removed vertices are never evaluated (two more host synchronisations; `info` in
        `self.last_mesh_clean`).  None (default): no cleaning.
        `simplify`: a dict of `mesh_simplify.simplify_mesh` keywords (`cell_size` in voxels, or `target_triangles`;
        `origin`); the simplification runs after the cleaning and before `vertex_attributes`, which is evaluated on the
        surviving vertices only (`info` in `self.last_mesh_simplify`).  None (default): no simplification.
        `cull`: a dict of `mesh_cull.cull_mesh` keywords, as in `extract_geometry`; the culling runs after the cleaning and
        before the simplification, so what no camera supports is neither evaluated nor baked (`info` in
        `self.last_mesh_cull`).  None (default): no culling.
        `bake`: a dict of `bake_textures` keywords (`size`, `chart`, `refine`, `max_step`, `threshold`, `albedo`, `slab`,
        `chunk`, `return_samples`; `threshold` defaults to this call's, `max_step` to one cell diagonal); the bake runs last,
        on the final vertices (cleaned, simplified and, where asked for, refined), and adds `uv` [T,3,2], `albedo_image`,
        `normal_image` and `bake` (the rest of `bake_textures`' result) to the dict.  None (default): nothing is added.
        `fill`: a dict of `mesh_fill.fill_holes` keywords (`max_edges`), as in `extract_geometry`; the filling runs after the
        last stage and before `vertex_attributes`, so the cap centroids get normals and colours, and `refine > 0` projects
        them onto the level set, like every other vertex (`info` in `self.last_mesh_fill`).  None (default): no filling."""
        mesh_pipeline.check_options(clean=clean, simplify=simplify, bake=bake, cull=cull, fill=fill)
        res = int(resolution)
        v, t = mesh_pipeline.device_mesh(self, bound_min, bound_max, res, threshold, sparse, brick, margin,
                                         {"clean": clean, "simplify": simplify, "cull": cull}, fill)
        at = self.vertex_attributes(grid_vertices=v, bounds=(bound_min, bound_max), resolution=res, threshold=threshold,
                                    refine=refine, max_step=max_step, chunk=chunk)
        if int(refine) > 0:
            vertices = at["points"].double()
        elif to_host:   # extract_geometry's rescaling, on the host as there
            vertices = mesh_pipeline.rescale_to_bounds_host(v.cpu().numpy(), bound_min, bound_max, res)
        else:
            vertices = mesh_pipeline.rescale_to_bounds_device(v, bound_min, bound_max, res)
        out = {"vertices": vertices, "triangles": t, "normals": at["normal"], "sdf": at["sdf"]}
        if "albedo" in at:
            out["albedo"], out["colors"] = at["albedo"], at["rgb"]
        baked = None
        if bake is not None:
            kw = dict(bake)
            kw.setdefault("threshold", threshold)
            if kw.get("max_step") is None:
                kw["max_step"] = mesh_pipeline.cell_diagonal(bound_min, bound_max, res)
            final = vertices if isinstance(vertices, torch.Tensor) else torch.from_numpy(vertices).to(t.device)
            baked = self.bake_textures(final, t, to_host=to_host, **kw)
        if to_host:
            out = {k: x.cpu().numpy() if isinstance(x, torch.Tensor) else x for k, x in out.items()}
        if baked is not None:
            for k in ("uv", "albedo_image", "normal_image"):
                out[k] = baked.pop(k)
            out["bake"] = baked
        return out
