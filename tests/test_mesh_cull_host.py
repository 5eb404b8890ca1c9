"""Host side of the mesh culling (rnb_mesh_view_votes / rnb_mesh_compact_triangles_* of include/rnbneus.h,
rnb_neus_fork_amd.mesh_cull): the numpy reference the GPU tests compare against (tests/mesh_cull_ref.py) on hand-made
cases and on the shared scene, `camera_projections` against the ray generation's own arithmetic, `binary_masks` on CPU
tensors, every argument check before anything touches a device, and the symbols declared, bound and exported.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rnb_neus_fork_amd as R
from rnb_neus_fork_amd import mesh_cull as M
from tests import mesh_cull_ref as F
from tests import raygen_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_INVALID, E_NULL = 0, -1, -4
IDENT = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])


# ------------------------------------------------------------------------------------------------------- the reference rule
def test_reference_rule_on_hand_made_points():
    """P = [I | 0]: (X, Y, Z) projects to (X / Z, Y / Z); a 4 x 3 frame (W = 4, H = 3) with one masked-out pixel"""
    H, W = 3, 4
    mask = np.ones((1, H, W), dtype=np.uint8)
    mask[0, 2, 1] = 0
    lo, hi = np.nextafter(-0.5, -1.0), np.nextafter(-0.5, 1.0)
    pts = np.array([[0.0, 0.0, 1.0],          # pixel (0, 0): seen
                    [-0.5, 0.0, 1.0],         # a = 0 exactly: in frame, pixel 0
                    [lo, 0.0, 1.0],           # just left of the frame
                    [hi, 0.0, 1.0],           # just inside
                    [W - 0.5, 0.0, 1.0],      # a = W exactly: out
                    [np.nextafter(W - 0.5, 0.0), 0.0, 1.0],
                    [1.0, 2.0, 1.0],          # the masked-out pixel
                    [2.0, 4.0, 2.0],          # the same pixel from twice the depth
                    [0.0, H - 0.5, 1.0],      # b = H exactly: out
                    [0.0, 0.0, 0.0],          # w = 0
                    [0.0, 0.0, -1.0],         # behind the camera
                    [np.nan, 0.0, 1.0], [0.0, np.inf, 1.0], [0.0, 0.0, np.inf]])
    none_v, none_t = np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32)
    eye = np.array([[0.0, 0.0, -1.0]])
    st, counts = F.view_votes(pts, IDENT[None], eye, mask, (H, W), none_v, none_t)
    assert st[0].tolist() == [3, 3, 0, 3, 0, 3, 1, 1, 0, 0, 0, 0, 0, 0]
    assert (counts.sum(axis=1) == 1).all() and counts.dtype == np.int32
    assert F.view_votes(pts, IDENT[None], eye, None, (H, W), none_v, none_t)[0][0].tolist() == [3, 3, 0, 3, 0, 3, 3, 3, 0, 0, 0, 0, 0, 0]
    px = F.frame_status(pts[[1, 3, 5]], IDENT, None, H, W)[2]
    assert px.tolist() == [0, 0, W - 1]


def test_reference_occlusion_on_two_parallel_triangles():
    """a camera at the origin looking down +z, a big triangle at z = 2 behind a small one at z = 1"""
    v = np.array([[-4.0, -4.0, 2.0], [8.0, -4.0, 2.0], [-4.0, 8.0, 2.0], [-0.25, -0.25, 1.0], [0.5, -0.25, 1.0], [-0.25, 0.5, 1.0]])
    t = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)
    P = np.array([[10.0, 0.0, 8.0, 0.0], [0.0, 10.0, 8.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
    pts = np.array([[0.0, 0.0, 2.0],       # on the far triangle behind the near one: occluded
                    [1.0, 1.0, 2.0],       # on the far triangle beside the near one: seen
                    [0.0, 0.0, 1.0],       # on the near triangle: seen (its own triangle is met at t = 1)
                    [0.0, 0.0, 0.0]])      # the eye itself: w = 0, out of frame
    eye = np.zeros((1, 3))
    st, counts = F.view_votes(pts, P[None], eye, None, (16, 16), v, t)
    assert st[0].tolist() == [F.OCCLUDED, F.SEEN, F.SEEN, F.OUT_OF_FRAME]
    assert F.view_votes(pts, P[None], eye, None, (16, 16), v, t, occlusion=False)[0][0].tolist() == [3, 3, 3, 0]
    # point == eye under a projection that keeps it in frame: the segment cannot be cast, status OCCLUDED
    Q = P.copy()
    Q[2, 3] = 1.0
    assert F.view_votes(pts[3:], Q[None], eye, None, (16, 16), v, t)[0][0].tolist() == [F.OCCLUDED]


def test_the_shared_scene_is_what_the_tests_assume():
    s = F.scene()
    c = s["counts"]
    outer, inner, floater = slice(0, 642), slice(642, 804), slice(804, 816)
    assert s["vertices"].shape == (816, 3) and s["triangles"].shape == (1620, 3)
    assert (c.sum(axis=1) == 6).all()
    assert (c[outer, F.OUTSIDE_MASK] == 0).all() and np.bincount(c[outer, F.SEEN]).tolist() == [0, 67, 335, 240]
    assert (c[inner, F.SEEN] == 0).all() and (c[inner, F.OUTSIDE_MASK] == 0).all()
    assert c[floater, F.OUTSIDE_MASK].min() >= 1 and c[floater, F.OUTSIDE_MASK].max() <= 2
    assert (s["counts_noocc"][inner, F.SEEN] == 6).all()
    v, t, vi, ti, _ = F.cull(s["vertices"], s["triangles"], s["projections"], s["eyes"], s["masks"], s["size"])
    assert np.array_equal(v, s["vertices"][outer]) and np.array_equal(t, s["triangles"][:1280])
    assert np.array_equal(vi, np.arange(642)) and np.array_equal(ti, np.arange(1280))


def test_reference_compaction():
    v = np.arange(18, dtype=np.float64).reshape(6, 3)
    t = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 0], [1, 9, 2], [5, 4, 3]], dtype=np.int32)
    vo, to, vi, ti = F.compact_triangles(v, t, [0, 1, 0, 1, 1])
    assert vi.tolist() == [2, 3, 4, 5] and ti.tolist() == [1, 4]             # triangle 3 holds index 9: dropped
    assert to.tolist() == [[0, 1, 2], [3, 2, 1]] and np.array_equal(vo, v[[2, 3, 4, 5]])
    vo, to, vi, ti = F.compact_triangles(v, t, np.zeros(5))
    assert vo.shape == (0, 3) and to.shape == (0, 3) and len(vi) == 0 and len(ti) == 0


# -------------------------------------------------------------------------------------------------------- camera_projections
def test_camera_projections_against_the_ray_generation():
    """a point at any depth on pixel (x, y)'s ray projects to that pixel: corners and centre of an odd-sized image"""
    H, W = 33, 47
    s = F.scene()
    kinv = s["intrinsics_inv"][0].copy()
    for pose in (s["pose"][0], s["pose"][3], s["pose"][4]):
        xs = np.array([0, W - 1, 0, W - 1, (W - 1) // 2], dtype=np.float64)
        ys = np.array([0, 0, H - 1, H - 1, (H - 1) // 2], dtype=np.float64)
        o, d, _, _ = raygen_ref.pixel_rays(kinv, pose, xs, ys, dtype=np.float64)
        P, eyes = R.camera_projections(torch.from_numpy(kinv), pose)
        assert P.shape == (1, 3, 4) and eyes.shape == (1, 3) and P.dtype == eyes.dtype == torch.float64
        assert np.array_equal(eyes[0].numpy(), pose[:3, 3])
        for depth in (0.1, 1.0, 7.5, 300.0):
            pts = o + depth * d
            x, y, w = F.project(pts, P[0].numpy())
            assert (w > 0).all()
            assert np.abs(x / w - xs).max() < 1e-9 and np.abs(y / w - ys).max() < 1e-9
            reaches, _, px, py = F.frame_status(pts, P[0].numpy(), None, H, W)
            assert reaches.all() and np.array_equal(px, xs.astype(np.int64)) and np.array_equal(py, ys.astype(np.int64))
    P, eyes = R.camera_projections(s["intrinsics_inv"], torch.from_numpy(s["pose"]).float())      # stacks, float32 in
    assert P.shape == (6, 3, 4) and np.abs(P.numpy() - s["projections"]).max() < 1e-5
    with pytest.raises(ValueError, match="pose"):
        R.camera_projections(kinv, np.eye(3))
    with pytest.raises(ValueError, match="intrinsics"):
        R.camera_projections(s["intrinsics_inv"][:2], s["pose"])


# -------------------------------------------------------------------------------------------------------------- binary_masks
@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16, torch.float32])
def test_binary_masks_on_cpu_tensors(dtype):
    full = {torch.uint8: 255, torch.uint16: 65535, torch.float32: 1.0}[dtype]
    half_below, half_above = ({torch.uint8: (127, 128), torch.uint16: (32767, 32768), torch.float32: (0.5, 0.500001)})[dtype]
    vals = np.zeros((2, 5, 6))
    vals[0, 0, 0], vals[0, 2, 3], vals[0, 4, 5], vals[1, 1, 1], vals[1, 3, 3] = full, half_above, full, half_below, half_above
    np_dtype = {torch.uint8: np.uint8, torch.uint16: np.uint16, torch.float32: np.float32}[dtype]
    m = torch.from_numpy(vals.astype(np_dtype))
    want = np.zeros((2, 5, 6), dtype=np.uint8)
    want[0, 0, 0] = want[0, 2, 3] = want[0, 4, 5] = want[1, 3, 3] = 1
    got = R.binary_masks(m)
    assert got.dtype == torch.uint8 and got.shape == (2, 5, 6) and np.array_equal(got.numpy(), want)
    four = torch.from_numpy(np.stack([vals, np.zeros_like(vals), np.zeros_like(vals)], axis=-1).astype(np_dtype))   # channel 0 decides
    assert np.array_equal(R.binary_masks(four).numpy(), want)
    assert np.array_equal(R.binary_masks(m, dilate=0).numpy(), want)
    grown = np.zeros_like(want)
    for c, y, x in zip(*np.nonzero(want)):
        grown[c, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 1                                       # clipped at the border, no wrap
    assert np.array_equal(R.binary_masks(m, dilate=1).numpy(), grown)
    assert grown[0, 0, 5] == 0 and grown[0, 1, 1] == 1 and grown[0, 3, 4] == 1
    assert int(R.binary_masks(m, threshold=1.0).sum()) == 0 and int(R.binary_masks(m, threshold=0.0).sum()) == 5


def test_binary_masks_arguments():
    m = torch.zeros(1, 2, 2, dtype=torch.uint8)
    for bad in (m[0], m.numpy(), m.to(torch.int64), m.to(torch.bool)):
        with pytest.raises(ValueError, match="masks"):
            R.binary_masks(bad)
    for thr in (-0.1, 1.5, "x", True):
        with pytest.raises(ValueError, match="threshold"):
            R.binary_masks(m, threshold=thr)
    for r in (-1, 1.5, True):
        with pytest.raises(ValueError, match="dilate"):
            R.binary_masks(m, dilate=r)
    assert R.binary_masks(torch.zeros(0, 4, 4)).shape == (0, 4, 4)


# ----------------------------------------------------------------------------------------------------------- argument checks
class _FakeIndex:
    def __init__(self, covers=True, device=torch.device("cpu")):
        self.covers, self.device = covers, device


def test_python_argument_checks_fire_on_the_host():
    s = F.scene()
    v, t = torch.from_numpy(s["vertices"]), torch.from_numpy(s["triangles"])
    P, e, masks = torch.from_numpy(s["projections"]), torch.from_numpy(s["eyes"]), torch.from_numpy(s["masks"])
    fake_rays = type("FakeRays", (), dict(pose_all=0, intrinsics_all_inv=0, masks=0, H=4, W=4))()
    # contradictory camera sources
    with pytest.raises(ValueError, match="not both"):
        R.cull_mesh(v, t, rays=fake_rays, projections=P, eyes=e)
    with pytest.raises(ValueError, match="not both"):
        R.cull_mesh(v, t, rays=fake_rays, masks=masks)
    with pytest.raises(ValueError, match="no cameras"):
        R.cull_mesh(v, t)
    with pytest.raises(ValueError, match="go together"):
        R.cull_mesh(v, t, projections=P)
    with pytest.raises(ValueError, match="DeviceRays"):
        R.cull_mesh(v, t, rays=object())
    with pytest.raises(ValueError, match="views"):
        R.cull_mesh(v, t, projections=P, eyes=e, views=[0])
    for bad in ("most", None, 1):
        with pytest.raises(ValueError, match="rule"):
            R.cull_mesh(v, t, projections=P, eyes=e, masks=masks, rule=bad)
    for name in ("max_outside", "min_seen"):
        for bad in (-1, 0.5, True):
            with pytest.raises(ValueError, match=name):
                R.cull_mesh(v, t, projections=P, eyes=e, masks=masks, **{name: bad})
    with pytest.raises(ValueError, match="dilate"):
        R.cull_mesh(v, t, projections=P, eyes=e, masks=masks, dilate=-2)
    with pytest.raises(ValueError, match="threshold"):
        R.cull_mesh(v, t, projections=P, eyes=e, masks=masks, threshold=2.0)
    with pytest.raises(ValueError, match="occlusion"):
        R.cull_mesh(v, t, projections=P, eyes=e, masks=masks, occlusion=1)
    with pytest.raises(ValueError, match="image_size"):
        R.cull_mesh(v, t, projections=P, eyes=e, image_size=(0, 4))
    with pytest.raises(RuntimeError, match="GPU tensors only"):                  # valid arguments: there is no CPU path
        R.cull_mesh(v, t, projections=P, eyes=e, masks=masks)
    # the renderer's cull=: the same checks, before the grid is evaluated
    from rnb_neus_fork_amd.mesh_pipeline import check_options

    def check(cull):
        check_options(cull=cull)
    check(None)
    check({"projections": P, "eyes": e, "masks": masks, "min_seen": 2, "rule": "any"})
    for bad, match in (({"rule": "all"}, "no cameras"), ({"projections": P, "eyes": e, "rule": "some"}, "rule"),
                       ({"projections": P, "eyes": e, "min_seen": -1}, "min_seen"),
                       ({"rays": fake_rays, "eyes": e}, "not both"), ({"projections": P, "eyes": e, "index": None}, "cull_mesh keywords"),
                       ({"projections": P, "eyes": e, "attributes": {}}, "cull_mesh keywords"), ([1], "cull_mesh keywords")):
        with pytest.raises(ValueError, match=match):
            check(bad)
    # view_votes
    idx, pts = _FakeIndex(), v[:5]
    for bad in (pts[:, :2], pts.numpy(), pts.to(torch.int64)):
        with pytest.raises(ValueError, match="points"):
            M.view_votes(idx, bad, P, e, masks)
    for tol in (-0.1, 1.0, float("nan"), "x", True):
        with pytest.raises(ValueError, match="rel_tol"):
            M.view_votes(idx, pts, P, e, masks, rel_tol=tol)
    with pytest.raises(ValueError, match="without grid="):
        M.view_votes(_FakeIndex(covers=False), pts, P, e, masks)
    for bad in (masks.float(), masks[0], masks.numpy()):
        with pytest.raises(ValueError, match="masks"):
            M.view_votes(idx, pts, P, e, bad)
    with pytest.raises(ValueError, match="image_size"):
        M.view_votes(idx, pts, P, e)
    with pytest.raises(ValueError, match="image_size"):
        M.view_votes(idx, pts, P, e, masks, image_size=(48, 47))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        M.view_votes(idx, pts, P, e, masks)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        M.view_votes(idx, pts.float(), P, e, image_size=(48, 48), occlusion=False, return_status=True)
    # compact_triangles
    keep = torch.ones(len(t), dtype=torch.bool)
    for bad in (keep[:-1], keep.float(), keep.numpy(), keep[:, None]):
        with pytest.raises(ValueError, match="keep"):
            R.compact_triangles(v, t, bad)
    with pytest.raises(ValueError, match="attribute"):
        R.compact_triangles(v, t, keep, {"a": torch.zeros(3)})
    with pytest.raises(ValueError, match="int32"):
        R.compact_triangles(v, t.long(), keep)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        R.compact_triangles(v, t, keep)


def _bins(dims=(4, 4, 4), cell=0.5, origin=(0.0, 0.0, 0.0)):
    return R.native.MeshBins((C.c_double * 3)(*origin), cell, (C.c_int32 * 3)(*dims), 0)


def test_library_argument_checks_come_before_any_launch():
    """Every call below returns before a stream or the device is touched: the pointers are made up."""
    lib = R.native.load()
    p = C.c_void_p(4096)           # never dereferenced on the host
    good, COVER, NOOCC = _bins(), R.native.MESH_BINS_COVER, R.native.CULL_NO_OCCLUSION

    def votes(pts=p, N=5, P=p, eyes=p, n_cam=2, masks=p, H=8, W=8, bins=good, cs=p, entries=p, E=9, corners=p, T=4, tol=1e-6,
              flags=COVER, counts=p, status=p):
        return lib.rnb_mesh_view_votes(pts, N, P, eyes, n_cam, masks, H, W, C.byref(bins) if bins is not None else None, cs,
                                       entries, E, corners, T, tol, flags, counts, status, None)

    assert votes(flags=0) == E_INVALID and b"RNB_MESH_BINS_COVER" in lib.rnb_last_error_string()
    assert votes(flags=NOOCC) == E_INVALID and votes(flags=COVER | 4) == E_INVALID and votes(flags=-1) == E_INVALID
    for kw in ("N", "n_cam", "E", "T"):
        assert votes(**{kw: -1}) == E_INVALID and votes(**{kw: 2 ** 31}) == E_INVALID, kw
    assert votes(H=0) == E_INVALID and votes(W=0) == E_INVALID and votes(H=-1, masks=None) == E_INVALID
    for tol in (-1e-9, 1.0, float("nan"), float("inf")):
        assert votes(tol=tol) == E_INVALID and b"rel_tol" in lib.rnb_last_error_string()
    assert votes(bins=_bins(dims=(0, 4, 4))) == E_INVALID and votes(bins=_bins(cell=0.0)) == E_INVALID
    assert votes(bins=None) == E_NULL and votes(counts=None) == E_NULL
    assert votes(pts=None) == E_NULL and votes(P=None) == E_NULL and votes(eyes=None) == E_NULL
    assert votes(cs=None) == E_NULL and votes(entries=None) == E_NULL and votes(corners=None) == E_NULL
    assert votes(N=0, pts=None, counts=None) == OK                                        # no point: nothing launched
    assert votes(N=0, flags=0) == E_INVALID and votes(N=0, tol=2.0) == E_INVALID         # still refused

    def count(tri=p, T=4, V=5, keep=p, ws=p, ws_bytes=1 << 20, counts=p):
        return lib.rnb_mesh_compact_triangles_count(tri, T, V, keep, ws, ws_bytes, counts, None)

    def emit(tri=p, T=4, vts=p, V=5, keep=p, ws=p, ws_bytes=1 << 20, nv=3, nt=2, vo=p, to=p, vi=p, ti=p):
        return lib.rnb_mesh_compact_triangles_emit(tri, T, vts, V, keep, ws, ws_bytes, nv, nt, vo, to, vi, ti, None)

    assert count(T=-1) == E_INVALID and count(V=2 ** 31) == E_INVALID and emit(T=2 ** 31) == E_INVALID
    assert count(tri=None) == E_NULL and count(keep=None) == E_NULL and count(ws=None) == E_NULL and count(counts=None) == E_NULL
    assert count(ws_bytes=16) == -2 and emit(ws_bytes=16) == -2                            # RNB_E_WORKSPACE
    assert emit(nv=6) == E_INVALID and emit(nt=5) == E_INVALID and emit(nv=-1) == E_INVALID
    assert emit(vi=None) == E_NULL and emit(to=None) == E_NULL and emit(ti=None) == E_NULL and emit(vo=None) == E_NULL
    need = C.c_int64()
    assert lib.rnb_mesh_clean_workspace_bytes(5, 4, C.byref(need)) == OK and need.value <= 1 << 20


def test_symbols_are_declared_bound_and_exported():
    lib = R.native.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnbneus.h")).read(), flags=re.S)
    for name, n_args in (("rnb_mesh_view_votes", 19), ("rnb_mesh_compact_triangles_count", 8), ("rnb_mesh_compact_triangles_emit", 14)):
        assert name in R.native.EXPORTED_SYMBOLS and hasattr(lib, name)
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/rnbneus.h"
        restype, argtypes = R.native._SIGNATURES[name]
        decls = [d.strip() for d in m.group(1).split(",")]
        assert restype is C.c_int and len(argtypes) == len(decls) == n_args, name
        for decl, ct in zip(decls, argtypes):
            if "rnb_mesh_bins*" in decl:
                assert ct is C.POINTER(R.native.MeshBins), decl
            elif "*" in decl or decl.startswith("rnb_stream_t"):
                assert ct is C.c_void_p, decl
            else:
                assert ct is {"int64_t": C.c_int64, "int32_t": C.c_int32, "size_t": C.c_size_t, "double": C.c_double}[decl.split()[0]], decl
    assert lib.rnb_abi_version() == 5 and R.native.ABI_VERSION == 5
    assert re.search(r"RNB_CULL_NO_OCCLUSION\s*=\s*2\b", header) and R.native.CULL_NO_OCCLUSION == 2
    assert re.search(r"RNB_CULL_OUT_OF_FRAME = 0, RNB_CULL_OUTSIDE_MASK = 1, RNB_CULL_OCCLUDED = 2, RNB_CULL_SEEN = 3", header)
    assert (R.native.CULL_OUT_OF_FRAME, R.native.CULL_OUTSIDE_MASK, R.native.CULL_OCCLUDED, R.native.CULL_SEEN) == (0, 1, 2, 3)
    assert M.STATUS_NAMES == ("out_of_frame", "outside_mask", "occluded", "seen")
    from rnb_neus_fork_amd import buildid
    assert "mesh_cull.hip" in buildid.HIP_SOURCES and buildid.EXTRA_FLAGS["mesh_cull.hip"] == ["-ffp-contract=off"]
    assert "csrc/mesh_raycast.hip.h" in [n for n, _ in buildid.source_files()], "the shared walk is hashed into the build id"
    assert {"cull_mesh", "camera_projections", "binary_masks", "compact_triangles"} <= set(R.__all__)
    assert hasattr(R.MeshIndex, "view_votes")
