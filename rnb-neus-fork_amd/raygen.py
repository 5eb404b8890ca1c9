"""Device-resident ray / target generation for `train_rnb`.

The reference prepares every step on the host: `Dataset.ps_gen_random_rays_at_view_on_all_lights`
(models/dataset.py:351-376) draws pixels with CPU `randint`, fancy-indexes the CPU-resident
`[n_images, n_lights, H, W, 3]` image stacks, copies the results to the GPU; `exp_runner.py:214-220` moves the
pixel indices back to the CPU to gather the per-pixel light directions; `near_far_from_sphere`
(dataset.py:448-458) follows.  `DeviceRays` keeps the stacks in HBM (226 MB each for DiLiGenT-MV, 7.5 GB each for
a 200-view 1024^2 capture: 288 GB of HBM hold them all) and produces everything a step consumes with one launch
(`rnb_gen_rays_at_view`).  Same method names, argument meaning and return tuple as the reference's `Dataset`, so
`exp_runner.py:174-180` works unchanged on it; `pixels_x` / `pixels_y` may be passed in so that tests can use the
reference's own draws.

Whole views (`validate_image`, `render_novel_image`: exp_runner.py:389-558) come from the same kernel on its grid front
(`rnb_gen_rays_grid`): `gen_rays_at` / `gen_rays_between` are the reference's methods, `view_rays` gives any range of
a view's rays together with near / far and the gathers at the rounded pixel, one launch per call.

Source mode (`DeviceRays.from_source_maps`): instead of the finished stacks of `Dataset.__init__` (27 floats and a mask
float per pixel) the object keeps the capture's normal, albedo and mask maps in their own dtype (7 bytes per pixel as
8-bit images) and `rnb_gen_rays_at_view_from_maps` / `rnb_gen_rays_grid_from_maps` (the kernel's map targets) compute
lights and colours for the pixels they are asked for (include/rnbneus.h states the arithmetic).  Every method keeps its
signature and return shapes; all of them launch through `DeviceRays._ray_launch`.  `cameras_from_projections` is the
reference's `load_K_Rt_from_P` without OpenCV."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import native


class _CameraRays(torch.autograd.Function):
    """`DeviceRays.sample` with a camera that requires grad: the forward is the one ray launch, the backward is
    `rnb_gen_rays_camera_bwd` (one launch).  rays_o, rays_d, near, far and, in source mode, the per-ray lights (the kernel
    rotates them with the pose) are differentiable in `pose` and `intrinsics_inv`; mask and colours are not, and
    stack-mode lights are gathers."""

    @staticmethod
    def forward(ctx, rays, v, px, py, warmup, pose, intrinsics_inv):
        pose_c, kinv_c = _camera_matrix(pose, rays.device), _camera_matrix(intrinsics_inv, rays.device)
        data, rgb, rgb_wu, lights, near, far = rays._launch(v, px, py, not warmup, warmup, not warmup, True, pose_c, kinv_c)
        rays_o, rays_d, mask, true_rgb = data[:, :3], data[:, 3:6], data[:, 6:7], rgb_wu if warmup else rgb
        rotated = lights is not None and rays.source_mode
        ctx.save_for_backward(pose_c, kinv_c, px, py, lights if rotated else None)
        ctx.n_lights = rays.n_lights if rotated else 0
        ctx.set_materialize_grads(False)     # an output the step does not use sends no adjoint: NULL at the entry point
        ctx.mark_non_differentiable(*(t for t in (mask, true_rgb, None if rotated else lights) if t is not None))
        return rays_o, rays_d, near, far, mask, true_rgb, lights

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, o_bar, d_bar, near_bar, far_bar, _mask_bar, _rgb_bar, lights_bar):
        pose, kinv, px, py, lights = ctx.saved_tensors
        B = px.numel()

        def adj(t, shape):
            return None if t is None else t.to(torch.float32).reshape(shape).contiguous()

        o_bar, d_bar = adj(o_bar, (B, 3)), adj(d_bar, (B, 3))
        near_bar, far_bar = adj(near_bar, (B,)), adj(far_bar, (B,))
        lights_bar = adj(lights_bar, (ctx.n_lights, B, 3)) if lights is not None else None
        pose_bar = torch.empty(4, 4, dtype=torch.float32, device=pose.device)
        kinv_bar = torch.empty_like(pose_bar) if ctx.needs_input_grad[6] else None
        native.same_device(pose, kinv, px, py, lights, o_bar, d_bar, near_bar, far_bar, lights_bar)
        with native.on_device(pose) as stream:
            native.check(native.load().rnb_gen_rays_camera_bwd(
                native.ptr(kinv), native.ptr(pose), native.ptr(px), native.ptr(py), B, native.ptr(lights), ctx.n_lights,
                native.ptr(o_bar), native.ptr(d_bar), native.ptr(lights_bar), native.ptr(near_bar), native.ptr(far_bar),
                native.ptr(pose_bar), native.ptr(kinv_bar), stream))
        return None, None, None, None, None, pose_bar if ctx.needs_input_grad[5] else None, kinv_bar


def _camera_matrix(t, device):
    """A [4,4] camera matrix as the kernels read it: detached float32, contiguous, on `device`."""
    t = torch.as_tensor(t).detach().to(device=device, dtype=torch.float32)
    if tuple(t.shape) != (4, 4):
        raise ValueError(f"a camera matrix is [4, 4], not {tuple(t.shape)}")
    return t.contiguous()


def _rotate(lights, rot):
    """rot [3,3] applied to the last axis of `lights` (a broadcast product and a 3-term sum: exact for the identity)."""
    return (lights.unsqueeze(-2) * rot).sum(-1)


class DeviceRays:
    def __init__(self, images, images_warmup, masks, light_directions, light_directions_warmup, intrinsics_all_inv,
                 pose_all, device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("DeviceRays: the image stacks must live on the GPU (there is no CPU path)")

        def put(t):
            return None if t is None else t.to(device=dev, dtype=torch.float32).contiguous()

        self.images = put(images)                                   # [V, L, H, W, 3]
        self.images_warmup = put(images_warmup)                     # [V, L, H, W, 3] or None
        self.masks = put(masks)                                     # [V, H, W, Cm]
        self.light_directions = put(light_directions)               # [V, L, H, W, 3] or None
        self.light_directions_warmup = put(light_directions_warmup)  # [V, L, 3] or None
        self.intrinsics_all_inv = put(intrinsics_all_inv)           # [V, 4, 4]
        self.pose_all = put(pose_all)                               # [V, 4, 4]
        self.device = dev
        self.n_images, self.n_lights, self.H, self.W = self.images.shape[:4]
        if self.masks.dim() == 3:
            self.masks = self.masks.unsqueeze(-1)
        if self.masks.shape[:3] != (self.n_images, self.H, self.W):
            raise ValueError(f"masks {tuple(self.masks.shape)} do not match images {tuple(self.images.shape)}")
        self.normals = self.albedos = None                          # source mode only (from_source_maps)
        self._refinement = None                                     # set_refinement

    @classmethod
    def from_dataset(cls, dataset, device="cuda"):
        """Takes the tensors of a constructed reference `Dataset` (models/dataset.py:219-239)."""
        return cls(dataset.images, getattr(dataset, "images_warmup", None), dataset.masks,
                   getattr(dataset, "light_directions", None), getattr(dataset, "light_directions_warmup", None),
                   dataset.intrinsics_all_inv, dataset.pose_all, device)

    @classmethod
    def from_source_maps(cls, normals, albedos, masks, intrinsics_all_inv, pose_all, device="cuda", tilt_deg=(0, 120, 240),
                         slant_deg=54.74, slant_warmup_deg=30):
        """Source mode: keeps the capture's maps on the device in their own dtype and computes lights and colours in the
        ray kernels.  `normals`, `albedos` [V,H,W,3] (RGB order, as the reference's `load_image` returns them; `albedos`
        None = the reference's `no_albedo`), `masks` [V,H,W] or [V,H,W,Cm]: torch tensors or numpy arrays of dtype uint8,
        uint16 (PNG values) or float32 (already decoded: normals in the reference's camera convention).  The lights are
        the reference's tilt / slant table (`light_tables`).  `images`, `images_warmup` and `light_directions` are None;
        `materialize` computes a view's."""
        normals, albedos, masks = _as_map(normals, "normals"), _as_map(albedos, "albedos"), _as_map(masks, "masks")
        if normals.dim() != 4 or normals.shape[-1] != 3:
            raise ValueError(f"normals {tuple(normals.shape)} are not [V, H, W, 3]")
        V, H, W = normals.shape[:3]
        if albedos is not None and (albedos.shape != normals.shape or albedos.dtype != normals.dtype):
            raise ValueError(f"albedos {tuple(albedos.shape)} {albedos.dtype} do not match normals {tuple(normals.shape)} "
                             f"{normals.dtype}")
        if masks.dim() == 3:
            masks = masks.unsqueeze(-1)
        if masks.dim() != 4 or masks.shape[:3] != (V, H, W) or masks.shape[3] < 1:
            raise ValueError(f"masks {tuple(masks.shape)} do not match normals {tuple(normals.shape)}")
        intrinsics_all_inv, pose_all = torch.as_tensor(intrinsics_all_inv), torch.as_tensor(pose_all)
        if intrinsics_all_inv.shape != (V, 4, 4) or pose_all.shape != (V, 4, 4):
            raise ValueError(f"intrinsics_all_inv {tuple(intrinsics_all_inv.shape)} / pose_all {tuple(pose_all.shape)} are not "
                             f"[{V}, 4, 4]")
        local, warm = light_tables(tilt_deg, slant_deg, slant_warmup_deg)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("DeviceRays: the source maps must live on the GPU (there is no CPU path)")
        self = cls.__new__(cls)
        self.device = dev
        self.images = self.images_warmup = self.light_directions = None
        self.normals = normals.to(dev).contiguous()                 # [V, H, W, 3] uint8 / uint16 / float32
        self.albedos = None if albedos is None else albedos.to(dev).contiguous()
        self.masks = masks.to(dev).contiguous()                     # [V, H, W, Cm]
        self.intrinsics_all_inv = intrinsics_all_inv.to(device=dev, dtype=torch.float32).contiguous()
        self.pose_all = pose_all.to(device=dev, dtype=torch.float32).contiguous()
        # dataset.py:207-211: pose[:3,:3] @ w_k in float64 (a float32 pose, the float64 lights), then float32
        rot = pose_all.detach().to(device="cpu", dtype=torch.float32)[:, :3, :3].double()
        self.light_directions_warmup = torch.einsum("vij,lj->vli", rot, torch.from_numpy(warm)).float().to(dev).contiguous()
        self.n_images, self.n_lights, self.H, self.W = V, local.shape[0], H, W
        self._local_lights, self._warmup_lights_cam = local.astype(np.float32), warm.astype(np.float32)
        self._source_structs = {}
        self._refinement = None
        return self

    @property
    def source_mode(self):
        return self.normals is not None

    def has_lights(self, warmup=False):
        """Whether the lights of `render_rnb_warmup` (`warmup`) or of `render_rnb` can be produced."""
        if warmup:
            return self.light_directions_warmup is not None
        return self.source_mode or self.light_directions is not None

    def resident_bytes(self):
        """Bytes this object holds in device memory (either mode)."""
        held = (self.images, self.images_warmup, self.masks, self.light_directions, self.light_directions_warmup,
                self.intrinsics_all_inv, self.pose_all, self.normals, self.albedos)
        return sum(t.numel() * t.element_size() for t in held if t is not None)

    def _source(self, v):
        """rnb_source_maps_t of view `v` (built once per view)."""
        st = self._source_structs.get(v)
        if st is None:
            st = native.SourceMaps()
            st.normals = self.normals[v].data_ptr()
            st.albedo = None if self.albedos is None else self.albedos[v].data_ptr()
            st.mask = self.masks[v].data_ptr()
            st.normals_type, st.mask_type = _TYPE_CODES[self.normals.dtype], _TYPE_CODES[self.masks.dtype]
            st.H, st.W, st.mask_channels, st.n_lights = self.H, self.W, self.masks.shape[-1], self.n_lights
            for k in range(self.n_lights):
                for c in range(3):
                    st.local_lights[k][c] = float(self._local_lights[k, c])
                    st.warmup_lights_cam[k][c] = float(self._warmup_lights_cam[k, c])
            self._source_structs[v] = st
        return st

    def materialize(self, img_idx):
        """Source mode: the reference's per-view tensors of view `img_idx`, computed by the whole-view kernel at
        resolution_level 1: a dict of `images`, `images_warmup`, `light_directions` [L,H,W,3] and `mask` [H,W,1]."""
        if not self.source_mode:
            raise ValueError("materialize: this DeviceRays already holds the stacks (it was not built from source maps)")
        L, H, W = self.n_lights, self.H, self.W
        main = self.view_rays(img_idx, resolution_level=1)
        warm = self.view_rays(img_idx, resolution_level=1, warmup=True)
        return {"images": main["true_rgb"].reshape(L, H, W, 3), "images_warmup": warm["true_rgb"].reshape(L, H, W, 3),
                "light_directions": main["lights_dir"].reshape(L, H, W, 3), "mask": main["mask"].reshape(H, W, 1)}

    # ------------------------------------------------------------------------------------------------
    def _pixels(self, batch_size, pixels_x, pixels_y):
        if pixels_x is None:
            # dataset.py:356-357 (drawn on the device here: the host generator is not on the path)
            pixels_x = torch.randint(0, self.W, (batch_size,), device=self.device)
            pixels_y = torch.randint(0, self.H, (batch_size,), device=self.device)
        else:
            if pixels_x.shape != (batch_size,) or pixels_y.shape != (batch_size,):
                raise ValueError("pixels_x / pixels_y must hold batch_size indices")
            on_host = not pixels_x.is_cuda and not pixels_y.is_cuda
            if on_host:   # host indices are checked on the host (an IndexError, like torch indexing)
                if batch_size and (int(pixels_x.min()) < 0 or int(pixels_x.max()) >= self.W
                                   or int(pixels_y.min()) < 0 or int(pixels_y.max()) >= self.H):
                    raise IndexError(f"pixel index out of range for a {self.H} x {self.W} image")
            pixels_x = pixels_x.to(device=self.device, dtype=torch.int64).contiguous()
            pixels_y = pixels_y.to(device=self.device, dtype=torch.int64).contiguous()
            if not on_host:   # device indices: asynchronous device-side check, no host round trip
                ok = (pixels_x >= 0) & (pixels_x < self.W) & (pixels_y >= 0) & (pixels_y < self.H)
                torch._assert_async(ok.all())
        return pixels_x, pixels_y

    def _ray_launch(self, v, n, front, want_rgb, want_warmup, want_lights, want_near_far, pose=None, intrinsics_inv=None,
                    view_pose=None, light=-1, targets=True):
        """The one ray launch: `n` rays of view `v` from one of two fronts, `front` = (pixels_x, pixels_y) ([n] int64 device
        tensors) or (tx, ty, first) (rays [first, first + n) of the row-major grid of the columns tx and the rows ty),
        with the targets of the lights `light` (-1 = all; the pixel front always takes all).  `pose`,
        `intrinsics_inv`, `view_pose` ([4,4] float32 contiguous device tensors): the camera of the rays and, for the grid
        front in source mode, the pose that rotates the view's lights; None = the view's stored ones (`pose`: `view_pose`).
        `targets` False: the pose-only view, no mask (0) and no gathers.  Allocates what is wanted and returns
        (data [n,7], rgb, rgb_wu, lights [Lo,n,3], near, far [n,1]), None where not wanted."""
        if not 0 <= v < self.n_images:
            raise IndexError(f"img_idx {v} out of range (n_images {self.n_images})")
        maps = targets and self.source_mode
        if not maps and want_warmup and self.images_warmup is None:
            raise ValueError("DeviceRays was built without images_warmup")
        if not maps and want_lights and self.light_directions is None:
            raise ValueError("DeviceRays was built without light_directions")
        L, Lo = self.n_lights, (self.n_lights if light < 0 else 1)
        f32 = dict(dtype=torch.float32, device=self.device)
        data = torch.empty(n, 7, **f32)
        rgb = torch.empty(Lo, n, 3, **f32) if want_rgb else None
        rgb_wu = torch.empty(Lo, n, 3, **f32) if want_warmup else None
        lights = torch.empty(Lo, n, 3, **f32) if want_lights else None
        near = torch.empty(n, 1, **f32) if want_near_far else None
        far = torch.empty(n, 1, **f32) if want_near_far else None
        view_pose = self.pose_all[v] if view_pose is None else view_pose
        camera = (native.ptr(self.intrinsics_all_inv[v] if intrinsics_inv is None else intrinsics_inv),
                  native.ptr(view_pose if pose is None else pose))
        out = (native.ptr(data), native.ptr(rgb), native.ptr(rgb_wu), native.ptr(lights), native.ptr(near), native.ptr(far))
        grid = len(front) == 3
        if grid:
            tx, ty, first, Wl, Hl = native.ptr(front[0]), native.ptr(front[1]), front[2], front[0].numel(), front[1].numel()
        else:
            px, py = native.ptr(front[0]), native.ptr(front[1])
        lib = native.load()
        with native.on_device(data) as stream:
            if maps:
                source = C.byref(self._source(v))
                if grid:
                    rc = lib.rnb_gen_rays_grid_from_maps(*camera, native.ptr(view_pose), tx, ty, Wl, Hl, first, n, source, light,
                                                         *out, stream)
                else:
                    rc = lib.rnb_gen_rays_at_view_from_maps(*camera, source, px, py, n, *out, stream)
            else:
                stacks = (native.ptr(self.images[v]) if want_rgb else None,
                          native.ptr(self.images_warmup[v]) if want_warmup else None,
                          native.ptr(self.masks[v]) if targets else None, self.masks.shape[-1],
                          native.ptr(self.light_directions[v]) if want_lights else None)
                if grid:
                    rc = lib.rnb_gen_rays_grid(*camera, tx, ty, Wl, Hl, first, n, *stacks, L, light, self.H, self.W, *out, stream)
                else:
                    rc = lib.rnb_gen_rays_at_view(*camera, *stacks, px, py, n, L, self.H, self.W, *out, stream)
            native.check(rc)
        return data, rgb, rgb_wu, lights, near, far

    def _launch(self, img_idx, pixels_x, pixels_y, want_rgb, want_warmup, want_lights, want_near_far, pose=None,
                intrinsics_inv=None):
        """The pixel front (`pose`, `intrinsics_inv`: as `_ray_launch` takes them)."""
        return self._ray_launch(int(img_idx), pixels_x.numel(), (pixels_x, pixels_y), want_rgb, want_warmup, want_lights,
                                want_near_far, pose, intrinsics_inv)

    # ------------------------------------------------------------------ the reference's Dataset methods
    def ps_gen_random_rays_at_view_on_all_lights(self, img_idx, batch_size, pixels_x=None, pixels_y=None):
        """models/dataset.py:351-376: returns (data [B,7], images_warmup [L,B,3], images [L,B,3], pixels_x,
        pixels_y), all on the device."""
        px, py = self._pixels(batch_size, pixels_x, pixels_y)
        data, rgb, rgb_wu, _, _, _ = self._launch(img_idx, px, py, True, self.source_mode or self.images_warmup is not None,
                                                  False, False)
        return data, rgb_wu, rgb, px, py

    def near_far_from_sphere(self, rays_o, rays_d):
        """models/dataset.py:448-458 (torch ops on device tensors, as in the reference)."""
        a = torch.sum(rays_d ** 2, dim=-1, keepdim=True)
        b = 2.0 * torch.sum(rays_o * rays_d, dim=-1, keepdim=True)
        mid = 0.5 * (-b) / a
        return mid - 1.0, mid + 1.0

    def light_directions_at(self, img_idx, pixels_y, pixels_x):
        """exp_runner.py:218: `light_directions[cbn, :, pixels_y, pixels_x, :]` -> [L, B, 3], without the host
        round trip of the pixel indices."""
        px, py = self._pixels(pixels_x.numel(), pixels_x, pixels_y)
        return self._launch(img_idx, px, py, False, False, True, False)[3]

    # ------------------------------------------------------------------ everything for one step, one launch
    def set_refinement(self, refinement):
        """A `CameraRefinement` (or None to remove it): `sample` then runs on `refinement.camera(v, ...)` of the view and
        is differentiable in the module's parameters; `view_rays` and `render_image` use the same cameras, detached.  The
        world-space lights this object holds were rotated by the stored poses, so they turn with the camera: the warm-up
        lights [L,3] and the gathered stack-mode lights are rotated by Exp(w_v) with a torch op (differentiable by torch),
        source-mode lights by the kernel with the refined pose.
        Everything else stays on the stored cameras and the unrotated lights: the reference's own methods
        `ps_gen_random_rays_at_view_on_all_lights` and `light_directions_at`, `materialize`, and `pose_between` /
        `gen_rays_between` (the interpolation runs between stored poses; `gen_rays_at` goes through `view_rays` and is
        refined).  `view_rays(pose=...)` without `img_idx` uses view 0's intrinsics as the reference does, refined when
        the module refines the focal length.  Do not mix the two groups in one step."""
        if refinement is not None and refinement.n_views != self.n_images:
            raise ValueError(f"the refinement holds {refinement.n_views} views, this DeviceRays {self.n_images}")
        self._refinement = refinement

    def _camera(self, v, pose=None, intrinsics_inv=None):
        """(pose, intrinsics_inv, rot) `sample` and `view_rays` run view `v` on: each matrix None where the stored one
        holds, `rot` = Exp(w_v) where the lights this object holds have to follow the camera (else None).  A `pose` or
        `intrinsics_inv` given by the caller is used as it is."""
        ref = self._refinement
        if ref is None or (pose is not None and intrinsics_inv is not None):
            return pose, intrinsics_inv, None
        r_pose, r_kinv = ref.camera(v, self.pose_all[v], self.intrinsics_all_inv[v])
        if ref.focal_log_scale is None:
            r_kinv = None
        rot = ref.rotation(v) if pose is None else None
        return r_pose if pose is None else pose, r_kinv if intrinsics_inv is None else intrinsics_inv, rot

    def sample(self, img_idx, batch_size, warmup=False, pixels_x=None, pixels_y=None, pose=None, intrinsics_inv=None):
        """Inputs of one `train_rnb` step (exp_runner.py:174-220) as a dict: rays_o, rays_d, near, far, mask,
        true_rgb, lights_dir (shaped for `render_rnb` / `render_rnb_warmup`), pixels_x, pixels_y.
        `pose`, `intrinsics_inv`: [4,4] device tensors to use instead of the view's stored camera (or of the one
        `set_refinement` composes).  Where a camera matrix requires grad, rays_o, rays_d, near, far and (source mode) the
        per-ray lights_dir carry a graph to it whose backward is one native launch (`rnb_gen_rays_camera_bwd`); mask,
        true_rgb and the pixels do not.  The gradients are those of this call's rays (shard-local under data parallelism).
        Otherwise the launch and the returned views are the same as without the two arguments.  A matrix that requires
        grad must be a float32 tensor on this object's device (its gradient is made there).  `pose[:3,:3]` is taken to be
        a rotation: the source-mode light adjoint recovers the camera-space light as R^T l, so a scaled or sheared pose
        gives rays and lights as computed but a wrong `pose.grad`."""
        px, py = self._pixels(batch_size, pixels_x, pixels_y)
        v = int(img_idx)
        if not 0 <= v < self.n_images:     # before `_camera` indexes the stacks (a negative index would wrap there)
            raise IndexError(f"img_idx {v} out of range (n_images {self.n_images})")
        if warmup and self.light_directions_warmup is None:
            raise ValueError("DeviceRays was built without light_directions_warmup")
        pose, intrinsics_inv, rot = self._camera(v, pose, intrinsics_inv)
        need_grad = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                                    for t in (pose, intrinsics_inv))
        if need_grad:
            for name, t in (("pose", pose), ("intrinsics_inv", intrinsics_inv)):
                if isinstance(t, torch.Tensor) and t.requires_grad and (t.device != self.device or t.dtype != torch.float32):
                    raise ValueError(f"sample: {name} requires grad, so it must be a float32 tensor on {self.device} "
                                     f"(got {t.dtype} on {t.device})")
            rays_o, rays_d, near, far, mask, true_rgb, lights = _CameraRays.apply(
                self, v, px, py, warmup, self.pose_all[v] if pose is None else pose,
                self.intrinsics_all_inv[v] if intrinsics_inv is None else intrinsics_inv)
        else:
            data, rgb, rgb_wu, lights, near, far = self._launch(
                v, px, py, not warmup, warmup, not warmup, True,
                None if pose is None else _camera_matrix(pose, self.device),
                None if intrinsics_inv is None else _camera_matrix(intrinsics_inv, self.device))
            rays_o, rays_d, mask, true_rgb = data[:, :3], data[:, 3:6], data[:, 6:7], rgb_wu if warmup else rgb
        if rot is not None and not need_grad:
            rot = rot.detach()
        if warmup:
            lights_dir = self.light_directions_warmup[v]
            if rot is not None:
                lights_dir = _rotate(lights_dir, rot)
            lights_dir = lights_dir.reshape(self.n_lights, 1, 1, 3)
        else:
            if rot is not None and not self.source_mode:
                lights = _rotate(lights, rot)
            lights_dir = lights.reshape(self.n_lights, batch_size, 1, 3)
        return {"rays_o": rays_o, "rays_d": rays_d, "mask": mask, "near": near, "far": far,
                "true_rgb": true_rgb, "lights_dir": lights_dir, "pixels_x": px, "pixels_y": py}

    # ------------------------------------------------------------------ whole views, one launch per call
    def _grid(self, resolution_level):
        l = int(resolution_level)
        if l < 1 or self.W // l < 1 or self.H // l < 1:
            raise ValueError(f"resolution_level {resolution_level} leaves no pixel of a {self.H} x {self.W} image")
        # dataset.py:307-308, made by torch so that the coordinates carry torch's bits (cached per level)
        cache = self.__dict__.setdefault("_grid_cache", {})
        if l not in cache:
            tx = torch.linspace(0, self.W - 1, self.W // l).to(self.device)
            ty = torch.linspace(0, self.H - 1, self.H // l).to(self.device)
            # (+ the coordinates of every ray of the row-major grid: view_rays returns slices of them)
            cache[l] = (tx, ty, tx.repeat(ty.numel()), ty.repeat_interleave(tx.numel()))
        return cache[l]

    def view_rays(self, img_idx=None, pose=None, resolution_level=1, light=None, warmup=False, first=0, count=None):
        """Rays `[first, first + count)` (default: all) of the row-major `H // l x W // l` grid of a view, with what a
        render of them consumes, one launch: a dict of `rays_o`, `rays_d` [n,3], `near`, `far` [n,1], `mask` [n,1],
        `lights_dir` (shaped for `render_rnb`: [Lo,n,1,3], or with `warmup` for `render_rnb_warmup`: [Lo,1,1,3]),
        `true_rgb` [Lo,n,3] (the nearest pixel of `images`, or of `images_warmup`), `pixels_x`, `pixels_y` [n] (the float
        grid coordinates), `H`, `W` (the grid's size).  `light`: one light index or None for all (Lo = 1 or n_lights).
        `pose` [4,4]: a camera-to-world pose other than a view's own (`gen_rays_between`); the intrinsics are then view
        0's (dataset.py:414) unless `img_idx` is given too, and mask / lights_dir / true_rgb are None when it is not."""
        tx, ty, px_all, py_all = self._grid(resolution_level)
        Wl, Hl = tx.numel(), ty.numel()
        first = int(first)
        n = Hl * Wl - first if count is None else int(count)
        if first < 0 or n < 1 or first + n > Hl * Wl:
            raise IndexError(f"rays [{first}, {first + n}) are not inside the {Hl} x {Wl} grid")
        gather = img_idx is not None
        v = int(img_idx) if gather else 0
        if not 0 <= v < self.n_images:
            raise IndexError(f"img_idx {v} out of range (n_images {self.n_images})")
        L = self.n_lights
        li = -1 if light is None else int(light)
        if not -1 <= li < L or (light is not None and li < 0):
            raise IndexError(f"light {light} out of range (n_lights {L})")
        Lo = L if li < 0 else 1
        view_pose = kinv = rot = None       # the view's stored camera, unless `set_refinement` composes one
        if self._refinement is not None:
            with torch.no_grad():           # (forward only: detached)
                view_pose, kinv, rot = self._camera(v)
            view_pose = None if view_pose is None else _camera_matrix(view_pose, self.device)
            kinv = None if kinv is None else _camera_matrix(kinv, self.device)
        if pose is None and not gather:
            raise ValueError("view_rays needs img_idx or pose")
        if pose is not None:
            pose = torch.as_tensor(pose).to(device=self.device, dtype=torch.float32).reshape(4, 4).contiguous()
        want_lights = gather and not warmup and self.has_lights()
        data, rgb, rgb_wu, lights, near, far = self._ray_launch(
            v, n, (tx, ty, first), gather and not warmup, gather and warmup, want_lights, True, pose, kinv, view_pose, li, gather)
        rgb = rgb_wu if warmup else rgb
        lights_dir = None
        if gather and warmup:
            if self.light_directions_warmup is None:
                raise ValueError("DeviceRays was built without light_directions_warmup")
            lw = self.light_directions_warmup[v]
            lw = lw if rot is None else _rotate(lw, rot)
            lights_dir = (lw if li < 0 else lw[li:li + 1]).reshape(Lo, 1, 1, 3)
        elif want_lights:
            if rot is not None and not self.source_mode:
                lights = _rotate(lights, rot)
            lights_dir = lights.reshape(Lo, n, 1, 3)
        return {"rays_o": data[:, :3], "rays_d": data[:, 3:6], "mask": data[:, 6:7] if gather else None, "near": near,
                "far": far, "true_rgb": rgb, "lights_dir": lights_dir, "pixels_x": px_all[first:first + n],
                "pixels_y": py_all[first:first + n], "H": Hl, "W": Wl}

    def gen_rays_at(self, img_idx, resolution_level=1):
        """models/dataset.py:300-326: (rays_o [Hl,Wl,3], rays_d [Hl,Wl,3], pixels_x [Hl,Wl], pixels_y [Hl,Wl]) on the
        device."""
        r = self.view_rays(img_idx, resolution_level=resolution_level)
        Hl, Wl = r["H"], r["W"]
        return (r["rays_o"].reshape(Hl, Wl, 3), r["rays_d"].reshape(Hl, Wl, 3), r["pixels_x"].reshape(Hl, Wl),
                r["pixels_y"].reshape(Hl, Wl))

    def pose_between(self, idx_0, idx_1, ratio):
        """The interpolated camera-to-world pose of `gen_rays_between` (float32 [4,4] numpy array, `interpolate_pose`)."""
        return interpolate_pose(self.pose_all[int(idx_0)].detach().cpu().numpy(),
                                self.pose_all[int(idx_1)].detach().cpu().numpy(), ratio)

    def gen_rays_between(self, idx_0, idx_1, ratio, resolution_level=1):
        """models/dataset.py:401-446: (rays_o [Hl,Wl,3], rays_d [Hl,Wl,3]) of the pose interpolated between two views
        (`pose_between`), with view 0's intrinsics as in the reference; the rays come from the same kernel."""
        r = self.view_rays(pose=self.pose_between(idx_0, idx_1, ratio), resolution_level=resolution_level)
        return r["rays_o"].reshape(r["H"], r["W"], 3), r["rays_d"].reshape(r["H"], r["W"], 3)


_TYPE_CODES = {torch.uint8: native.SOURCE_U8, torch.uint16: native.SOURCE_U16, torch.float32: native.SOURCE_F32}


def _as_map(a, name):
    """A source map as a torch tensor of one of the three element types (None passes)."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    if not isinstance(t, torch.Tensor) or t.dtype not in _TYPE_CODES:
        raise ValueError(f"{name} must be uint8, uint16 or float32 (got {getattr(t, 'dtype', type(t).__name__)})")
    return t


def light_tables(tilt_deg=(0, 120, 240), slant_deg=54.74, slant_warmup_deg=30):
    """The two light tables of `Dataset.gen_light_directions` (models/dataset.py:255-266) as float64 [L,3] arrays:
    u_k = -(sin s cos t_k, sin s sin t_k, cos s) with s = `slant_deg` (the main phase's lights in the per-pixel frame) and
    with s = `slant_warmup_deg` (the warm-up phase's camera-space lights).  rnb_source_maps_t takes them rounded to
    float32."""
    tilt = np.radians(np.asarray(tilt_deg, dtype=np.float64).reshape(-1))
    if not 1 <= tilt.shape[0] <= native.MAX_RENDER_LIGHTS:
        raise ValueError(f"{tilt.shape[0]} lights: a render takes 1 to {native.MAX_RENDER_LIGHTS}")

    def table(slant_deg):
        slant = np.radians(np.full(tilt.shape, float(slant_deg)))
        return (-np.array([np.sin(slant) * np.cos(tilt), np.sin(slant) * np.sin(tilt), np.cos(slant)])).transpose().copy()

    return table(slant_deg), table(slant_warmup_deg)


def _rq3(m):
    """RQ decomposition of a 3x3 matrix (float64): m = r q, r upper triangular with a positive diagonal, q orthogonal."""
    flip = np.eye(3)[::-1]
    q0, r0 = np.linalg.qr((flip @ m).T)
    r, q = flip @ r0.T @ flip, flip @ q0.T
    sign = np.where(np.diag(r) < 0, -1.0, 1.0)
    return r * sign[None, :], q * sign[:, None]


def cameras_from_projections(world_mats, scale_mats):
    """`(intrinsics_all [V,4,4], pose_all [V,4,4])` (float32 tensors) from a capture's `world_mat_i` / `scale_mat_i`
    (cameras.npz), as models/dataset.py:13-46 and :197-205 derive them with OpenCV's decomposeProjectionMatrix:
    P = (world_mat @ scale_mat)[:3,:4] in float32, P[:3,:3] = K R by an RQ decomposition (float64, K's diagonal made
    positive), intrinsics = K / K[2,2], pose[:3,:3] = R^T, pose[:3,3] = the camera centre (P (C, 1) = 0)."""
    intrinsics, poses = [], []
    for world_mat, scale_mat in zip(world_mats, scale_mats):
        P = (np.asarray(world_mat, dtype=np.float32) @ np.asarray(scale_mat, dtype=np.float32))[:3, :4].astype(np.float64)
        K, R = _rq3(P[:, :3])
        intr, pose = np.eye(4), np.eye(4)
        intr[:3, :3] = K / K[2, 2]
        pose[:3, :3] = R.T
        pose[:3, 3] = -np.linalg.solve(P[:, :3], P[:, 3])
        intrinsics.append(intr)
        poses.append(pose)
    return (torch.from_numpy(np.stack(intrinsics)).float(), torch.from_numpy(np.stack(poses)).float())


def interpolate_pose(pose_0, pose_1, ratio):
    """The interpolated camera-to-world pose of models/dataset.py:418-437 from two float32 [4,4] poses, built on the host
    as there: both poses inverted in float32, their rotations slerped (float64, the arithmetic of scipy's Slerp: R0 times
    the rotation of R0^T R1 with its angle scaled by `ratio`) and their translations lerped, assembled in float32 and
    inverted.  Returns a float32 [4,4] numpy array."""
    pose_0 = np.linalg.inv(np.asarray(pose_0, dtype=np.float32))
    pose_1 = np.linalg.inv(np.asarray(pose_1, dtype=np.float32))
    rot = _slerp(pose_0[:3, :3].astype(np.float64), pose_1[:3, :3].astype(np.float64), float(ratio))
    pose = np.diag([1.0, 1.0, 1.0, 1.0]).astype(np.float32)
    pose[:3, :3] = rot
    pose[:3, 3] = ((1.0 - ratio) * pose_0 + ratio * pose_1)[:3, 3]
    return np.linalg.inv(pose)


def _quat_from_matrix(m):
    """Unit quaternion (x, y, z, w) of a 3x3 matrix's nearest rotation (float64; the largest-component branch)."""
    u, _, vt = np.linalg.svd(m)
    m = u @ np.diag([1.0, 1.0, np.linalg.det(u @ vt)]) @ vt
    t = np.trace(m)
    c = [m[0, 0], m[1, 1], m[2, 2], t]
    k = int(np.argmax(c))
    q = np.empty(4)
    if k == 3:
        q[:] = (m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], 1.0 + t)
    else:
        i, j, l = k, (k + 1) % 3, (k + 2) % 3
        q[i] = 1.0 - t + 2.0 * m[i, i]
        q[j] = m[j, i] + m[i, j]
        q[l] = m[l, i] + m[i, l]
        q[3] = m[l, j] - m[j, l]
    return q / np.linalg.norm(q)


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def _quat_to_matrix(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _slerp(r0, r1, t):
    """Rotation matrix R0 exp(t log(R0^T R1)) (numpy float64): spherical interpolation between two rotations along the
    shorter arc, t = 0 -> R0, t = 1 -> R1."""
    q0, q1 = _quat_from_matrix(r0), _quat_from_matrix(r1)
    d = _quat_mul(q0 * np.array([-1.0, -1.0, -1.0, 1.0]), q1)     # q0^-1 q1
    if d[3] < 0:
        d = -d
    s = np.linalg.norm(d[:3])
    angle = 2.0 * np.arctan2(s, d[3])
    if s < 1e-300:
        return _quat_to_matrix(q0)
    half = 0.5 * t * angle
    step = np.concatenate([d[:3] / s * np.sin(half), [np.cos(half)]])
    return _quat_to_matrix(_quat_mul(q0, step))
