"""The mesh culling entry points between guard bands (tests/guard_bands.py), by the rule of tests/test_gpu_guard_geometry.py:
every call runs once on ordinary allocations and once under guarded() with its inputs passed through guard(); both bands of
every allocation must still hold their pattern, the registry must have seen the buffers the call is known to make, and every
result must equal the unguarded run bit for bit (integer atomics only: the votes are reproducible).  Under guarded() the
body of every torch.empty holds the pattern, so the votes [N,4] — which the call itself must zero — and every compacted
array are at the same time checked for words the kernels never wrote.  One positive control: an output handed out short
trips the bands.  Every case prints one line starting with GUARD."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from tests import guard_bands as GB
from tests import mesh_cull_ref as F
from tests import mesh_distance_ref as MD
from tests import mesh_large_shapes as L
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device

pytestmark = pytest.mark.gpu

u8 = torch.uint8


@pytest.fixture(autouse=True)
def _release():
    yield
    GB.release()


def _dev(x, g=lambda t: t):
    if x is None or isinstance(x, (int, float, tuple, str)):
        return x
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return g(t.to(device()))


def _twice(tag, call, ins):
    """call(inputs on the device) on ordinary allocations, then between bands: intact, and the same bits"""
    t0 = time.perf_counter()
    clean = call({k: _dev(v) for k, v in ins.items()})
    torch.cuda.synchronize()
    with GB.guarded() as s:
        got = call({k: _dev(v, GB.guard) for k, v in ins.items()})
        torch.cuda.synchronize()
        GB.assert_intact(tag)
    GB.assert_same(tag, clean, got)
    print(f"GUARD cull {tag}: {len(s.registry)} guarded allocations, {time.perf_counter() - t0:.2f} s")
    return s, got


def _made(s, what, **kw):
    got = [e for e in s.seen(**kw) if e.how != "guard"]
    assert got, f"{what}: no guarded allocation of {kw}"
    return got


def _scene_inputs():
    s = F.scene()
    return {k: s[k] for k in ("vertices", "triangles", "projections", "eyes", "masks")}


def _votes(R, x, n, cams, **kw):
    index = R.MeshIndex(x["vertices"], x["triangles"])
    out = index.view_votes(x["vertices"][:n], x["projections"][:cams], x["eyes"][:cams], x["masks"][:cams], **kw)
    return {k: out[k] for k in ("counts", "status") if k in out}       # (the four columns are views of counts)


@pytest.mark.parametrize("n,cams", [(816, 6), (65, 1), (1, 6)])
def test_view_votes(R, n, cams):
    """with and without the status array; N past a wavefront by one point, and one point"""
    s0 = F.scene()

    def call(x):
        return _votes(R, x, n, cams, return_status=True), _votes(R, x, n, cams), _votes(R, x, n, cams, occlusion=False)

    s, (with_status, plain, noocc) = _twice(f"view_votes N={n} C={cams}", call, _scene_inputs())
    _made(s, "counts", shape=(n, 4), dtype=torch.int32)
    _made(s, "status", shape=(cams, n), dtype=u8)
    assert len(s.seen(shape=(n, 4), dtype=torch.int32)) == 3 and len(s.seen(shape=(cams, n), dtype=u8)) == 1
    assert np.array_equal(with_status["status"].cpu().numpy(), s0["status"][:cams, :n])
    assert torch.equal(plain["counts"], with_status["counts"]) and bool((noocc["counts"].sum(dim=1) == cams).all())


def test_compact_triangles(R):
    v, t = MD.torus_mesh()
    keep = np.random.default_rng(5).uniform(size=len(t)) < 0.4
    ws = C.c_int64()
    R.native.check(R.native.load().rnb_mesh_clean_workspace_bytes(len(v), len(t), C.byref(ws)))

    def call(x):
        return (R.compact_triangles(x["v"], x["t"], x["keep"], {"id": torch.arange(len(v), device=device())}),
                R.compact_triangles(x["v"], x["t"], torch.zeros_like(x["keep"])), R.compact_triangles(x["v"], x["t"], torch.ones_like(x["keep"])))

    s, (some, none, every) = _twice("compact_triangles torus", call, {"v": v, "t": t, "keep": keep})
    want = F.compact_triangles(v, t, keep)
    assert np.array_equal(some["vertices"].cpu().numpy(), want[0]) and np.array_equal(some["triangles"].cpu().numpy(), want[1])
    _made(s, "workspace", nbytes=ws.value, dtype=u8)
    _made(s, "vertices", shape=tuple(want[0].shape), dtype=torch.float64)
    _made(s, "triangles", shape=tuple(want[1].shape), dtype=torch.int32)
    _made(s, "vertex_index", shape=(len(want[2]),), dtype=torch.int64)
    _made(s, "triangle_index", shape=(len(want[3]),), dtype=torch.int64)
    assert none["triangles"].shape == (0, 3) and every["triangles"].shape == (len(t), 3)


def test_compact_triangles_past_the_first_chunk_of_the_block_sum_scan(R):
    """SHEET of tests/mesh_large_shapes.py: 1,027 triangle tile sums and 515 vertex tile sums in the workspace, so the one
    workgroup that scans them stores through a second chunk of the first array and none of the second"""
    d = L.big("SHEET")
    v, t = d["vertices"], d["triangles"]
    assert L.tiles(len(t)) == 1027 and L.tiles(len(v)) == 515 and L.chunks(len(t)) == 2 and L.chunks(len(v)) == 1
    keep = L.random_keep(len(t))
    ws = C.c_int64()
    R.native.check(R.native.load().rnb_mesh_clean_workspace_bytes(len(v), len(t), C.byref(ws)))
    s, got = _twice("compact_triangles SHEET", lambda x: R.compact_triangles(x["v"], x["t"], x["keep"]), {"v": v, "t": t, "keep": keep})
    nv, nt = got["info"]["n_vertices"][1], got["info"]["n_triangles"][1]
    assert nt == int(keep.sum()) and int(got["triangle_index"][-1]) >= L.LINE
    _made(s, "workspace", nbytes=ws.value, dtype=u8)
    _made(s, "vertices", shape=(nv, 3), dtype=torch.float64)
    _made(s, "triangles", shape=(nt, 3), dtype=torch.int32)
    _made(s, "triangle_index", shape=(nt,), dtype=torch.int64)


def test_cull_mesh(R):
    def call(x):
        cams = dict(projections=x["projections"], eyes=x["eyes"])
        return (R.cull_mesh(x["vertices"], x["triangles"], masks=x["masks"] * 255, **cams),
                R.cull_mesh(x["vertices"], x["triangles"], masks=x["masks"] * 255, occlusion=False, dilate=1, rule="any", **cams),
                R.cull_mesh(x["vertices"], x["triangles"], image_size=(48, 48), max_outside=2, **cams))

    s, (outer, both, nomask) = _twice("cull_mesh scene", call, _scene_inputs())
    assert outer["triangles"].shape == (1280, 3) and both["triangles"].shape[0] >= 1600 and nomask["triangles"].shape[0] > 1280
    _made(s, "votes", shape=(816, 4), dtype=torch.int32)
    _made(s, "outer sphere", shape=(642, 3), dtype=torch.float64)
    _made(s, "its triangles", shape=(1280, 3), dtype=torch.int32)


@pytest.mark.parametrize("what", ["counts", "status", "triangles"])
def test_an_output_handed_out_short_trips_the_bands(R, what):
    """the positive control: the same calls with one output counted 4 bytes short — the kernel's last store lands in the band"""
    ins = _scene_inputs()
    shape = {"counts": (816, 4), "status": (6, 816), "triangles": (1280, 3)}[what]
    with GB.guarded(shortchange=(shape, 4)) as s:
        x = {k: _dev(v, GB.guard) for k, v in ins.items()}
        if what == "triangles":
            R.cull_mesh(x["vertices"], x["triangles"], projections=x["projections"], eyes=x["eyes"], masks=x["masks"] * 255)
        else:
            _votes(R, x, 816, 6, return_status=True)
        torch.cuda.synchronize()
        bad = s.damaged()
    assert len(bad) == 1 and bad[0]["band"] == "trailing" and tuple(bad[0]["shape"]) == shape, bad
    assert bad[0]["first"] >= bad[0]["nbytes"] and bad[0]["last"] < bad[0]["nbytes"] + 4, bad
    print(f"GUARD cull positive control {what}: bytes {bad[0]['first']} .. {bad[0]['last']} of {list(shape)} reported")
