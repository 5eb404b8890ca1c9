"""Thin host runtime over the C ABI: weight packing, workspaces, point-wise network calls.
Everything here is plumbing (torch owns the memory and the stream); all arithmetic is native."""
from __future__ import annotations

import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import native
from .fields import RenderingNetwork, SDFNetwork, mlp_struct, model_desc


def _require_cuda(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU: the renderer has no CPU path "
                           "(librnbneus_hip.so is the only implementation)")


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


def packed_floats(desc) -> int:
    n = C.c_int64()
    native.check(native.load().rnb_packed_floats(C.byref(desc), C.byref(n)))
    return n.value


def pack_weights(desc, sdf: SDFNetwork | None, color: RenderingNetwork | None, device, zero=False) -> torch.Tensor:
    """rnb_weightnorm_fwd: effective weights of both MLPs in the library's packed layout (zero: the rows of an absent
    network are zeros instead of uninitialised memory)."""
    lib = native.load()
    packed = (torch.zeros if zero else torch.empty)(packed_floats(desc), dtype=torch.float32, device=device)
    sp = mlp_struct(sdf.lins(), sdf.weight_norm) if sdf is not None else None
    cp = mlp_struct(color.lins(), color.weight_norm) if color is not None else None
    with native.on_device(packed) as stream:
        native.check(lib.rnb_weightnorm_fwd(C.byref(desc), C.byref(sp) if sp is not None else None,
                                            C.byref(cp) if cp is not None else None, native.ptr(packed), stream))
    return packed


def points_workspace(desc, n, device):
    return native.workspace("points", device, C.byref(desc), n)


def sdf_forward(desc, packed, pts, with_feature):
    _require_cuda(pts, "points")
    pts = _f32c(pts).reshape(-1, 3)
    n = pts.shape[0]
    sdf = torch.empty(n, 1, dtype=torch.float32, device=pts.device)
    feat = torch.empty(n, desc.sdf_d_out - 1, dtype=torch.float32, device=pts.device) if with_feature else None
    if n > 0:
        native.same_device(packed, pts)
        ws = points_workspace(desc, n, pts.device)
        with native.on_device(pts) as stream:
            native.check(native.load().rnb_sdf_forward(C.byref(desc), native.ptr(packed), native.ptr(pts), n,
                                                       native.ptr(sdf), native.ptr(feat), native.ptr(ws), ws.numel(),
                                                       stream))
    return torch.cat([sdf, feat], dim=-1) if with_feature else sdf


def sdf_gradient(desc, packed, pts):
    _require_cuda(pts, "points")
    pts = _f32c(pts).reshape(-1, 3)
    n = pts.shape[0]
    grad = torch.empty(n, 3, dtype=torch.float32, device=pts.device)
    if n > 0:
        native.same_device(packed, pts)
        ws = points_workspace(desc, n, pts.device)
        with native.on_device(pts) as stream:
            native.check(native.load().rnb_sdf_gradient(C.byref(desc), native.ptr(packed), native.ptr(pts), n,
                                                        native.ptr(grad), None, native.ptr(ws), ws.numel(), stream))
    return grad


def color_forward(desc, packed, pts, normals, feats):
    _require_cuda(pts, "points")
    pts = _f32c(pts).reshape(-1, 3)
    normals = _f32c(normals).reshape(-1, 3)
    feats = _f32c(feats).reshape(pts.shape[0], -1)
    n = pts.shape[0]
    out = torch.empty(n, desc.col_d_out, dtype=torch.float32, device=pts.device)
    if n > 0:
        native.same_device(packed, pts, normals, feats)
        ws = points_workspace(desc, n, pts.device)
        with native.on_device(pts) as stream:
            native.check(native.load().rnb_color_forward(C.byref(desc), native.ptr(packed), native.ptr(pts),
                                                         native.ptr(normals), native.ptr(feats), n, native.ptr(out),
                                                         native.ptr(ws), ws.numel(), stream))
    return out


def mesh_vertex_attrs(desc, packed, points=None, grid_vertices=None, bound_min=None, bound_max=None, resolution=0,
                      level=0.0, refine=0, max_step=0.0, albedo=False, swap_rb=True, chunk=65536):
    """rnb_mesh_vertex_attrs: per-vertex `points` [V,3], `sdf` [V,1], `gradient` [V,3], `normal` [V,3] and with `albedo`
    `albedo` [V,col_d_out] and `rgb` [V,3] uint8, for fp32 `points` or float64 `grid_vertices` (+ bounds and resolution).
    The library chunks the vertices through one workspace of min(chunk, V rounded up to 64) points."""
    src = grid_vertices if grid_vertices is not None else points
    _require_cuda(src, "vertices")
    dev = src.device
    gv = pts = None
    if grid_vertices is not None:
        gv = grid_vertices.detach().to(torch.float64).reshape(-1, 3).contiguous()
    else:
        pts = _f32c(points).reshape(-1, 3)
    V = (gv if gv is not None else pts).shape[0]
    f32 = dict(dtype=torch.float32, device=dev)
    out = {"points": torch.empty(V, 3, **f32), "sdf": torch.empty(V, 1, **f32), "gradient": torch.empty(V, 3, **f32),
           "normal": torch.empty(V, 3, **f32)}
    if albedo:
        out["albedo"] = torch.empty(V, desc.col_d_out, **f32)
        out["rgb"] = torch.empty(V, 3, dtype=torch.uint8, device=dev)
    if V == 0:
        return out
    chunk = min(int(chunk), (V + 63) // 64 * 64)
    a = native.MeshVertexArgs()
    a.grid_vertices, a.points, a.V = native.ptr(gv), native.ptr(pts), V
    if gv is not None:
        for d in range(3):
            a.bound_min[d], a.bound_max[d] = float(bound_min[d]), float(bound_max[d])
        a.resolution = int(resolution)
    a.level, a.refine, a.max_step = float(level), int(refine), float(max_step)
    a.flags = (native.MESH_ALBEDO if albedo else 0) | (native.MESH_SWAP_RB if swap_rb else 0)
    a.points_out, a.sdf_out = native.ptr(out["points"]), native.ptr(out["sdf"])
    a.gradient_out, a.normal_out = native.ptr(out["gradient"]), native.ptr(out["normal"])
    a.albedo_out, a.rgb_out = native.ptr(out.get("albedo")), native.ptr(out.get("rgb"))
    lib = native.load()
    ws = torch.empty(native.workspace_bytes("mesh_vertex", C.byref(desc), chunk, a.flags), dtype=torch.uint8, device=dev)
    native.same_device(packed, gv, pts)
    with native.on_device(dev) as stream:
        native.check(lib.rnb_mesh_vertex_attrs(C.byref(desc), native.ptr(packed), C.byref(a), chunk, native.ptr(ws),
                                               ws.numel(), stream))
    return out


def texture_sample_points(vertices, triangles, s, first, count, points_out, bad_out=None):
    """rnb_texture_sample_points: the lattice samples first .. first + count - 1 of the atlas with chart size s into
    `points_out` [count,3] fp32 (enqueued; `bad_out` [1] int64 is added to)."""
    native.same_device(vertices, triangles, points_out, bad_out)
    with native.on_device(triangles) as stream:
        native.check(native.load().rnb_texture_sample_points(native.ptr(vertices), vertices.shape[0], native.ptr(triangles),
                                                             triangles.shape[0], int(s), int(first), int(count),
                                                             native.ptr(points_out), native.ptr(bad_out), stream))


def texture_pack(vertices, triangles, s, cols, W, H, rgb=None, normal=None, albedo=True, normals=True, texel_sample=True):
    """rnb_texture_pack: (albedo_image [H,W,4] uint8 or None, normal_image [H,W,4] uint8 or None, texel_sample [H,W] int32
    or None) from the per-sample `rgb` [N,3] uint8 and `normal` [N,3] fp32 (enqueued, no host read)."""
    dev = native.same_device(vertices, triangles, rgb, normal)
    lay = native.TextureLayout(int(s), int(cols), int(W), int(H))
    a_img = torch.empty(H, W, 4, dtype=torch.uint8, device=dev) if albedo else None
    n_img = torch.empty(H, W, 4, dtype=torch.uint8, device=dev) if normals else None
    t_smp = torch.empty(H, W, dtype=torch.int32, device=dev) if texel_sample else None
    with native.on_device(dev) as stream:
        native.check(native.load().rnb_texture_pack(native.ptr(vertices), vertices.shape[0], native.ptr(triangles),
                                                    triangles.shape[0], C.byref(lay), native.ptr(rgb), native.ptr(normal),
                                                    native.ptr(a_img), native.ptr(n_img), native.ptr(t_smp), stream))
    return a_img, n_img, t_smp


class StandaloneSDF:
    """Context for calling an SDFNetwork outside a renderer (exp_runner.py:607-610 style)."""

    def __init__(self, sdf: SDFNetwork):
        self.sdf = sdf
        self.desc = model_desc(sdf, None)

    def _packed(self):
        dev = self.sdf.lin0.bias.device
        _require_cuda(self.sdf.lin0.bias, "SDFNetwork parameters")
        return pack_weights(self.desc, self.sdf, None, dev)

    def sdf_forward(self, x, with_feature):
        return sdf_forward(self.desc, self._packed(), x, with_feature)

    def sdf_gradient(self, x):
        return sdf_gradient(self.desc, self._packed(), x)


def _color_desc(color: RenderingNetwork, sdf_hidden, sdf_multires=0):
    """Descriptor of an albedo-net call without a renderer: a minimal placeholder SDF shape (one hidden layer of
    `sdf_hidden`) completes it; only the albedo rows of the packed buffer are written and read."""
    d = native.ModelDesc()
    d.sdf_d_in, d.sdf_d_out, d.sdf_d_hidden, d.sdf_n_layers = 3, color.d_feature + 1, sdf_hidden, 1
    d.sdf_skip_in, d.sdf_multires, d.sdf_scale, d.sdf_weight_norm = -1, sdf_multires, 1.0, 1
    d.col_d_feature, d.col_d_in, d.col_d_out = color.d_feature, color.d_in, color.d_out
    d.col_d_hidden, d.col_n_layers, d.col_multires_view = color.d_hidden, color.n_layers, color.multires_view
    d.col_squeeze_out, d.col_weight_norm = int(bool(color.squeeze_out)), int(color.weight_norm)
    d.n_samples, d.n_importance, d.up_sample_steps = 64, 0, 1
    return d


def standalone_color(color: RenderingNetwork, pts, normals, feats):
    """RenderingNetwork.forward without a renderer."""
    d = _color_desc(color, 32)
    _require_cuda(color.lin0.bias, "RenderingNetwork parameters")
    packed = pack_weights(d, None, color, color.lin0.bias.device)
    return color_forward(d, packed, pts, normals, feats)


# ---------------------------------------------------------------------------------------------------------------------
# opt-in autograd of the direct network calls (SDFNetwork / RenderingNetwork.set_autograd): the forward keeps the render
# path's per-point state, the backward is the render backward below the composite, seeded with the point adjoints
# (rnb_sdf_backward / rnb_color_backward), + rnb_weightnorm_bwd to the leaves, as in renderer._FinePass
# ---------------------------------------------------------------------------------------------------------------------
def points_grad_workspace(desc, n, flags, device):
    return native.workspace("points_grad", device, C.byref(desc), n, flags)


def _leaf_grads(desc, net, packed_grad, color):
    """rnb_weightnorm_bwd: the packed gradient -> one tensor per leaf of `net` (net.leaves() order)."""
    leaves = net.leaves()
    flat = torch.empty(sum(p.numel() for p in leaves), dtype=torch.float32, device=packed_grad.device)
    views, off = {}, 0
    for p in leaves:
        views[id(p)] = flat[off:off + p.numel()]
        off += p.numel()
    params = mlp_struct(net.lins(), net.weight_norm)
    grads = mlp_struct(net.lins(), net.weight_norm, grads=views)
    sp, sg = (None, None) if color else (C.byref(params), C.byref(grads))
    cp, cg = (C.byref(params), C.byref(grads)) if color else (None, None)
    with native.on_device(packed_grad) as stream:
        native.check(native.load().rnb_weightnorm_bwd(C.byref(desc), sp, cp, native.ptr(packed_grad), sg, cg, stream))
    return [views[id(p)].view_as(p) for p in leaves]


def _check_backward(ctx, what):
    if ctx.ws is None:
        raise RuntimeError(f"{what}: backward called a second time on the same call (the saved per-point state is released "
                           "after the first backward, retain_graph is not supported); re-run the forward")


def _once(what):
    if torch.is_grad_enabled():
        raise RuntimeError(f"{what} is differentiable once (its backward is native): backward(create_graph=True) through it "
                           "is not supported")


def _grad_in(g, n, width):
    return None if g is None else g.detach().to(torch.float32).reshape(n, width).contiguous()


_SDF_FLAGS = {"sdf": 0, "feature": native.POINTS_FEATURE, "normal": native.POINTS_NORMAL}


class _SDFPoints(torch.autograd.Function):
    """SDFNetwork.forward / .sdf ("feature" / "sdf": outputs sdf [n,1] (+ feature [n,F])) and .gradient ("normal": d sdf / d x
    [n,3]) with a native backward in every SDF leaf and x."""

    @staticmethod
    def forward(ctx, net, mode, x, *leaves):
        flags = _SDF_FLAGS[mode]
        desc = model_desc(net, None)
        dev = x.device
        pts = _f32c(x).reshape(-1, 3)
        n = pts.shape[0]
        f32 = dict(dtype=torch.float32, device=dev)
        sdf = torch.empty(n, 1, **f32)
        feat = torch.empty(n, desc.sdf_d_out - 1, **f32) if mode == "feature" else None
        nrm = torch.empty(n, 3, **f32) if mode == "normal" else None
        packed = pack_weights(desc, net, None, dev)
        ws = points_grad_workspace(desc, n, flags, dev)
        if n > 0:
            native.same_device(packed, pts)
            with native.on_device(dev) as stream:
                native.check(native.load().rnb_sdf_forward_save(C.byref(desc), native.ptr(packed), native.ptr(pts), n, flags,
                                                                native.ptr(sdf), native.ptr(feat), native.ptr(nrm),
                                                                native.ptr(ws), ws.numel(), stream))
        ctx.net, ctx.mode, ctx.desc, ctx.flags, ctx.n = net, mode, desc, flags, n
        ctx.packed, ctx.ws, ctx.x_shape, ctx.x_dtype = packed, ws, x.shape, x.dtype
        ctx.set_materialize_grads(False)
        if mode == "feature":
            return sdf, feat
        return nrm if mode == "normal" else sdf

    @staticmethod
    def backward(ctx, *gouts):
        _once(f"SDFNetwork ({ctx.mode})")
        return _SDFPoints._backward(ctx, *gouts)

    @staticmethod
    @once_differentiable
    def _backward(ctx, *gouts):
        _check_backward(ctx, "SDFNetwork")
        n, desc, dev = ctx.n, ctx.desc, ctx.ws.device
        g_sdf = g_feat = g_nrm = None
        if ctx.mode == "feature":
            g_sdf, g_feat = _grad_in(gouts[0], n, 1), _grad_in(gouts[1], n, desc.sdf_d_out - 1)
        elif ctx.mode == "sdf":
            g_sdf = _grad_in(gouts[0], n, 1)
        else:
            g_nrm = _grad_in(gouts[0], n, 3)
        want_x = ctx.needs_input_grad[2]
        xbar = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_x else None
        packed_grad = torch.empty_like(ctx.packed)
        with native.on_device(dev) as stream:
            native.check(native.load().rnb_sdf_backward(C.byref(desc), native.ptr(ctx.packed), n, ctx.flags, native.ptr(g_sdf),
                                                        native.ptr(g_feat), native.ptr(g_nrm), native.ptr(packed_grad),
                                                        native.ptr(xbar), native.ptr(ctx.ws), ctx.ws.numel(), stream))
        grads = _leaf_grads(desc, ctx.net, packed_grad, color=False)
        ctx.ws = ctx.packed = None
        if xbar is not None:
            xbar = xbar.reshape(ctx.x_shape).to(ctx.x_dtype)
        return (None, None, xbar) + tuple(grads)


class _ColorPoints(torch.autograd.Function):
    """RenderingNetwork.forward (mode no_view_dir) with a native backward in every albedo-net leaf, points, normals and
    features (view_dirs are not an input: the reference encodes and discards them)."""

    @staticmethod
    def forward(ctx, net, pts, normals, feats, *leaves):
        desc = _color_desc(net, 256, 6)   # (a placeholder the fused kernels accept: the shipped albedo net runs fused)
        dev = pts.device
        p = _f32c(pts).reshape(-1, 3)
        n = p.shape[0]
        nr = _f32c(normals).reshape(n, 3)
        ft = _f32c(feats).reshape(n, -1)
        out = torch.empty(n, desc.col_d_out, dtype=torch.float32, device=dev)
        packed = pack_weights(desc, None, net, dev, zero=True)
        ws = points_grad_workspace(desc, n, native.POINTS_COLOR, dev)
        if n > 0:
            native.same_device(packed, p, nr, ft)
            with native.on_device(dev) as stream:
                native.check(native.load().rnb_color_forward_save(C.byref(desc), native.ptr(packed), native.ptr(p),
                                                                  native.ptr(nr), native.ptr(ft), n, native.ptr(out),
                                                                  native.ptr(ws), ws.numel(), stream))
        ctx.net, ctx.desc, ctx.n, ctx.packed, ctx.ws = net, desc, n, packed, ws
        ctx.shapes = ((pts.shape, pts.dtype), (normals.shape, normals.dtype), (feats.shape, feats.dtype))
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, g_out):
        _once("RenderingNetwork")
        return _ColorPoints._backward(ctx, g_out)

    @staticmethod
    @once_differentiable
    def _backward(ctx, g_out):
        _check_backward(ctx, "RenderingNetwork")
        n, desc, dev = ctx.n, ctx.desc, ctx.ws.device
        f32 = dict(dtype=torch.float32, device=dev)
        want = ctx.needs_input_grad[1:4]
        pbar = torch.empty(n, 3, **f32) if want[0] else None
        nbar = torch.empty(n, 3, **f32) if want[1] else None
        fbar = torch.empty(n, desc.col_d_feature, **f32) if want[2] else None
        packed_grad = torch.empty_like(ctx.packed)
        if g_out is None:
            g_out = torch.zeros(n, desc.col_d_out, **f32)
        g = _grad_in(g_out, n, desc.col_d_out)
        with native.on_device(dev) as stream:
            native.check(native.load().rnb_color_backward(C.byref(desc), native.ptr(ctx.packed), n, native.ptr(g),
                                                          native.ptr(packed_grad), native.ptr(fbar), native.ptr(nbar),
                                                          native.ptr(pbar), native.ptr(ctx.ws), ctx.ws.numel(), stream))
        grads = _leaf_grads(desc, ctx.net, packed_grad, color=True)
        ctx.ws = ctx.packed = None
        ins = tuple(None if t is None else t.reshape(shape).to(dtype) for t, (shape, dtype) in zip((pbar, nbar, fbar), ctx.shapes))
        return (None,) + ins + tuple(grads)


def sdf_autograd(net: SDFNetwork, x, mode):
    _require_cuda(x, "points")
    _require_cuda(net.lin0.bias, "SDFNetwork parameters")
    return _SDFPoints.apply(net, mode, x, *net.leaves())


def color_autograd(net: RenderingNetwork, pts, normals, feats):
    for t, name in ((pts, "points"), (normals, "normals"), (feats, "feature_vectors"), (net.lin0.bias, "RenderingNetwork parameters")):
        _require_cuda(t, name)
    return _ColorPoints.apply(net, pts, normals, feats, *net.leaves())
