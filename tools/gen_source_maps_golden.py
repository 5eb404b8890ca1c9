"""Golden vectors of the reference's dataset preparation: tests/golden/source_maps_small.npz.

TEST INFRASTRUCTURE ONLY, run on the CPU where the reference checkout is available (RNB_REFERENCE, as
oracle/gen_golden.py).  Records what `Dataset.__init__` (models/dataset.py:100-239) makes of a capture's normal, albedo
and mask images: the stacks `images`, `images_warmup`, `light_directions`, `light_directions_warmup` and `masks`.

The reference's own `Dataset.gen_light_directions` is called, without and with normals (the per-pixel SVD, :255-298):
that is the part that cannot be restated.  Driving `Dataset.__init__` itself is not practical: it reads a configuration
object, globs PNG files, decodes them and the projection matrices with OpenCV (absent here) and moves tensors to a CUDA
device, so nearly every line would run against a stub.  Its arithmetic between the calls is restated here line by line
instead, with the dtypes it has there: the decode of `load_image` / `load_normal` (:48-68, float32), the masks (:134-136),
the shading (:157-182, float32 normals against float64 lights), the rotation to world space (:207-216, the float32 pose)
and the final `.astype(np.float32)` (:219-223).  `cv2` and `icecream` are inert placeholder modules.  No reference source
is stored.

The capture: V = 3 views of H x W = 13 x 11, 8-bit normals, albedo and masks; for view 1 also an independently drawn
16-bit copy of normals and albedo.  Every view's normals hold camera-facing unit normals (quantised), 12 back-facing
ones (decoded n_z > 0), the all-zero PNG value (decodes to (-1, 1, 1)) and clearly non-unit ones (lengths 0.5 and about
1.4); the masks hold 0, 127, 128 and 255.  A decoded n_z is (2 v - M) / M with M odd, so it is never 0.  Poses are random
rotations with a translation of length 3, intrinsics a pinhole camera with distinct focal lengths.

    python tools/gen_source_maps_golden.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "source_maps_small.npz")
V, H, W = 3, 13, 11
N_BACK = 12


def reference_dataset():
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")
    import_reference()
    from models.dataset import Dataset  # type: ignore
    return Dataset.__new__(Dataset)


def encode(normals, maximum):
    """PNG values of camera-convention normals (the inverse of load_normal, models/dataset.py:59-68, rounded)."""
    flipped = normals * np.array([1.0, -1.0, -1.0])
    return np.clip(np.rint((flipped + 1.0) / 2.0 * maximum), 0, maximum)


def draw_normals(rng, maximum, dtype):
    """[H,W,3] PNG values of one view"""
    n = rng.normal(size=(H * W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    n[:, 2] = -np.abs(n[:, 2]) - 0.02                      # camera-facing
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    order = rng.permutation(H * W)
    back, short, long_ = order[:N_BACK], order[N_BACK:N_BACK + 4], order[N_BACK + 4:N_BACK + 8]
    n[back, 2] = -n[back, 2]                               # back-facing: decoded n_z > 0
    n[short] *= 0.5
    n[long_] = np.clip(n[long_] * 1.4, -1.0, 1.0)
    v = encode(n, maximum)
    v[order[N_BACK + 8]] = 0                               # the all-zero PNG value
    return v.reshape(H, W, 3).astype(dtype)


def decode_image(values):
    """An RGB array of PNG values as models/dataset.py:48-57 scales it: float32 values / float32 maximum"""
    return values / np.float32(np.iinfo(values.dtype).max)


def decode_normal(values):
    """models/dataset.py:59-68: [0, 1] -> [-1, 1] in float32, y and z negated"""
    return (decode_image(values) * 2.0 - 1.0) * np.array([1.0, -1.0, -1.0], dtype=np.float32)


def stacks(ds, normal_values, albedo_values, pose):
    """What models/dataset.py:154-182 and :207-222 make of views [n,H,W,3] with float32 poses [n,4,4]: images,
    images_warmup, light_directions (world), light_directions_warmup; albedo_values None = no_albedo.  float32 normals
    and albedo against the float64 lights give float64 products, rounded to float32 at the end."""
    normals = decode_normal(normal_values)
    assert normals.dtype == np.float32
    albedo = np.ones_like(normals) if albedo_values is None else decode_image(albedo_values)
    warm_cam = ds.gen_light_directions().transpose()                 # [L,3] float64
    lights_cam = ds.gen_light_directions(normals)                    # [n,L,H,W,3]: the reference's per-pixel SVD
    assert warm_cam.dtype == np.float64 and lights_cam.dtype == np.float64
    shade_warm = np.maximum((normals[:, None] * warm_cam[None, :, None, None, :]).sum(axis=-1), 0)
    shade = np.maximum((normals[:, None] * lights_cam).sum(axis=-1), 0)
    images_warmup = albedo[:, None] * shade_warm[..., None]
    images = albedo[:, None] * shade[..., None]
    rot = pose[:, :3, :3]
    lights_warm_world = np.stack([(rot[i] @ warm_cam.T).T for i in range(len(rot))])
    lights_world = np.stack([(rot[i] @ lights_cam[i].reshape(-1, 3).T).T.reshape(lights_cam[i].shape)
                             for i in range(len(rot))])
    return (images.astype(np.float32), images_warmup.astype(np.float32), lights_world.astype(np.float32),
            lights_warm_world.astype(np.float32))


def main():
    ds = reference_dataset()
    rng = np.random.default_rng(20240917)
    normals_u8 = np.stack([draw_normals(rng, 255, np.uint8) for _ in range(V)])
    albedo_u8 = rng.integers(0, 256, size=(V, H, W, 3)).astype(np.uint8)
    masks_u8 = rng.choice(np.array([0, 127, 128, 255, 40, 200], dtype=np.uint8), size=(V, H, W))
    masks_u8[:, 0, :4] = np.array([0, 127, 128, 255], dtype=np.uint8)
    normals_u16 = draw_normals(rng, 65535, np.uint16)
    albedo_u16 = rng.integers(0, 65536, size=(H, W, 3)).astype(np.uint16)

    q = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(V)])
    q *= np.sign(np.linalg.det(q))[:, None, None]                                # proper rotations
    pose = np.tile(np.eye(4), (V, 1, 1))
    pose[:, :3, :3] = q
    c = rng.normal(size=(V, 3))
    pose[:, :3, 3] = 3.0 * c / np.linalg.norm(c, axis=-1, keepdims=True)
    pose = pose.astype(np.float32)
    K = np.tile(np.eye(4), (V, 1, 1))
    K[:, 0, 0], K[:, 1, 1] = 14.0 + rng.random(V), 15.0 + rng.random(V)
    K[:, 0, 2], K[:, 1, 2] = W / 2.0, H / 2.0
    intrinsics_inv = np.linalg.inv(K).astype(np.float32)

    images, images_warmup, lights, lights_warmup = stacks(ds, normals_u8, albedo_u8, pose)
    na_images, na_warmup, _, _ = stacks(ds, normals_u8[:1], None, pose[:1])
    u16_images, u16_warmup, u16_lights, _ = stacks(ds, normals_u16[None], albedo_u16[None], pose[1:2])
    masks = np.where(masks_u8 / 255.0 > 0.5, 1.0, 0.0).astype(np.float32)[..., None]          # :134-136, :223

    decoded = decode_normal(normals_u8)
    assert int((decoded[..., 2] > 0).sum(axis=(1, 2)).min()) >= 10 and bool((normals_u8 == 0).all(axis=-1).any())
    assert set(np.unique(masks_u8)) >= {0, 127, 128, 255}
    out = {"normals_u8": normals_u8, "albedo_u8": albedo_u8, "masks_u8": masks_u8, "normals_u16": normals_u16,
           "albedo_u16": albedo_u16, "intrinsics_inv": intrinsics_inv, "pose": pose,
           "warmup_lights_cam": ds.gen_light_directions().transpose().copy(),
           "images": images, "images_warmup": images_warmup, "light_directions": lights,
           "light_directions_warmup": lights_warmup, "masks": masks,
           "noalbedo_images": na_images[0], "noalbedo_images_warmup": na_warmup[0],
           "u16_images": u16_images[0], "u16_images_warmup": u16_warmup[0], "u16_light_directions": u16_lights[0]}
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
