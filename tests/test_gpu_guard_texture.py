"""The texture-bake entry points between guard bands (tests/guard_bands.py): rnb_texture_sample_points, rnb_texture_pack
and NeuSRenderer.bake_textures.

The rule of tests/test_gpu_guard_geometry.py: every call runs once on ordinary allocations and once under guarded() with
its inputs passed through guard(); both bands of every allocation must still hold their pattern, the registry must have
seen the buffers the call is known to make, and every result must equal the unguarded run bit for bit (integer arithmetic
and one integer counter: the calls are reproducible).  The shapes are the ones that end inside something: an odd number of
triangles (a half-empty last cell), a sample range that ends inside a triangle, an image whose last rows and columns are
margin.  Every case prints one line starting with GUARD."""
import time

import numpy as np
import pytest
import torch

from tests import guard_bands as GB
from tests import mesh_attrs_util as U
from tests import texture_bake_ref as F
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device

pytestmark = pytest.mark.gpu

# three triangles (odd T) over five vertices, inside the model's box
VERTS = np.array([[0.0, 0.0, 0.1], [0.4, 0.0, 0.2], [0.0, 0.4, -0.1], [0.4, 0.4, 0.05], [0.7, 0.2, 0.3]])
TRIS = np.array([[0, 1, 2], [2, 1, 3], [1, 4, 3]], dtype=np.int32)


@pytest.fixture(autouse=True)
def _release():
    yield
    GB.release()


def _dev(x, g=lambda t: t):
    return g(torch.from_numpy(np.ascontiguousarray(x)).to(device()))


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
    print(f"GUARD texture {tag}: {len(s.registry)} guarded allocations, {time.perf_counter() - t0:.2f} s")
    return s, got


def _made(s, what, **kw):
    got = [e for e in s.seen(**kw) if e.how != "guard"]
    assert got, f"{what}: no guarded allocation of {kw}"
    return got


@pytest.mark.parametrize("s", [1, 7])
def test_sample_points_range_ending_inside_a_triangle(R, s):
    n_s = F.n_samples(s)
    first, count = n_s // 2 + 1, n_s + 1          # starts and ends inside a triangle

    def call(x):
        pts = torch.empty(count, 3, dtype=torch.float32, device=device())
        bad = torch.zeros(1, dtype=torch.int64, device=device())
        R.runtime.texture_sample_points(x["v"], x["t"], s, first, count, pts, bad)
        return pts, bad

    g, (pts, bad) = _twice(f"sample_points s={s} [{first}, {first + count})", call, {"v": VERTS, "t": TRIS})
    want, _ = F.sample_points(VERTS, TRIS, s, first, count)
    assert np.array_equal(pts.cpu().numpy().view(np.uint32), want.view(np.uint32)) and int(bad.cpu()) == 0
    _made(g, "points_out", shape=(count, 3), dtype=torch.float32)
    _made(g, "bad_out", shape=(1,), dtype=torch.int64)


@pytest.mark.parametrize("s", [1, 7])
def test_pack_into_an_image_with_margins(R, s):
    n_s = F.n_samples(s)
    c = s + 5
    W = H = 2 * c + 3                             # 2 x 2 cells, three texels of margin right and below; the fourth cell half empty
    L = dict(s=s, c=c, cols=2, rows=1, W=W, H=H, samples_per_triangle=n_s)
    rng = np.random.default_rng(s)
    rgb = rng.integers(0, 256, (3 * n_s, 3), dtype=np.uint8)
    nrm = rng.uniform(-1.0, 1.0, (3 * n_s, 3)).astype(np.float32)

    def call(x):
        return R.runtime.texture_pack(x["v"], x["t"], s, 2, W, H, x["rgb"], x["nrm"])

    g, (a_img, n_img, smp) = _twice(f"pack s={s} {W}x{H}", call, {"v": VERTS, "t": TRIS, "rgb": rgb, "nrm": nrm})
    wa, wn, ws = F.pack(L, VERTS, TRIS, rgb, nrm)
    assert np.array_equal(a_img.cpu().numpy(), wa) and np.array_equal(n_img.cpu().numpy(), wn) and np.array_equal(smp.cpu().numpy(), ws)
    assert (ws[:, 2 * c:] == -1).all() and (ws[2 * c:] == -1).all() and (ws[c:2 * c, c:2 * c] == -1).all()
    assert len(_made(g, "images", shape=(H, W, 4), dtype=torch.uint8)) == 2
    _made(g, "texel_sample", shape=(H, W), dtype=torch.int32)


@pytest.mark.parametrize("which", ["sharp", "tiny"])
def test_bake_textures(R, which):
    """three triangles at chart 3 (30 samples: less than one 64-point tile) and chart 7 (108: a tile and a part) in two
    slabs of 64, into a forced image with margins"""
    ren = U.renderer(R, which, device())
    for chart, size, slab in ((3, 19, 1 << 20), (7, 27, 64)):
        def call(x):
            o = ren.bake_textures(x["v"], x["t"], chart=chart, size=size, slab=slab, return_samples=True, to_host=False)
            o["layout"] = o["layout"].asdict()        # (numbers: what guard_bands.flatten compares)
            return o

        g, out = _twice(f"bake_textures {which} chart={chart} size={size} slab={slab}", call, {"v": VERTS, "t": TRIS})
        N = 3 * F.n_samples(chart)
        assert out["info"] == {"samples": N, "bad_triangles": 0, "slabs": -(-N // slab)}
        _made(g, "normal samples", shape=(N, 3), dtype=torch.float32)
        _made(g, "rgb samples", shape=(N, 3), dtype=torch.uint8)
        assert len(_made(g, "images", shape=(size, size, 4), dtype=torch.uint8)) == 2
        lay = R.AtlasLayout(**out["layout"])
        assert lay.cols == 2 and lay.W == size > 2 * lay.c
        wa, wn, ws = F.pack(lay.asdict(), VERTS, TRIS, U.quantize_rgb(out["albedo"]).numpy(), out["normal"].cpu().numpy())
        assert np.array_equal(out["albedo_image"].cpu().numpy(), wa) and np.array_equal(out["normal_image"].cpu().numpy(), wn)
        assert np.array_equal(out["texel_sample"].cpu().numpy(), ws)
