"""Host side of the texture bake (rnb_texture_* of include/rnbneus.h, rnb_neus_fork_amd.texture_bake, the OBJ / PNG writers
of mesh_io): the symbols are declared, bound and exported together, every argument check comes before anything touches a
device, the layout arithmetic, the ownership of texels and the bilinear footprint of the numpy reference the GPU tests
compare against (tests/texture_bake_ref.py), and the file round trips.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rnb_neus_fork_amd as R
from rnb_neus_fork_amd import texture_bake as TB
from tests import texture_bake_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rnb_texture_sample_points", "rnb_texture_pack")


def test_symbols_are_declared_bound_and_exported():
    lib = R.native.load()
    header = open(os.path.join(ROOT, "include", "rnbneus.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMBOLS:
        assert name in R.native.EXPORTED_SYMBOLS
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/rnbneus.h"
        restype, argtypes = R.native._SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(m.group(1).split(",")), f"{name}: argument count"
        for decl, ct in zip(m.group(1).split(","), argtypes):
            decl = decl.strip()
            if "*" in decl or decl.startswith("rnb_stream_t"):
                assert ct in (C.c_void_p, C.POINTER(R.native.TextureLayout)), (name, decl)
            else:
                assert ct is (C.c_int32 if decl.startswith("int32_t") else C.c_int64), (name, decl)
        assert hasattr(lib, name)
    assert re.search(r"int32_t\s+s;.*int32_t\s+cols;.*int32_t\s+W,\s*H;", header, flags=re.S), "rnb_texture_layout's fields"
    assert [f[0] for f in R.native.TextureLayout._fields_] == ["s", "cols", "W", "H"] and C.sizeof(R.native.TextureLayout) == 16
    assert lib.rnb_abi_version() == 5 and R.native.ABI_VERSION == 5
    from rnb_neus_fork_amd import buildid
    assert "texture_bake.hip" in buildid.HIP_SOURCES and "-ffp-contract=off" in buildid.EXTRA_FLAGS["texture_bake.hip"]
    for name in ("atlas_layout", "atlas_uv", "sample_texture", "write_obj", "read_obj", "write_png", "read_png"):
        assert name in R.__all__ and callable(getattr(R, name)), name
    assert callable(R.NeuSRenderer.bake_textures)


def test_argument_checks_come_before_any_launch():
    """Every call below returns before a stream or the device is touched: the pointers are made up (a call that got as
    far as a launch would need a device)."""
    lib = R.native.load()
    p = C.c_void_p(4096)           # never dereferenced on the host

    def sample(V=8, T=4, verts=p, tri=p, s=2, first=0, count=24, pts=p, bad=p):
        return lib.rnb_texture_sample_points(verts, V, tri, T, s, first, count, pts, bad, None)

    def pack(V=8, T=4, verts=p, tri=p, s=2, cols=2, W=14, H=7, rgb=p, nrm=p, ai=p, ni=p, ts=p):
        return lib.rnb_texture_pack(verts, V, tri, T, C.byref(R.native.TextureLayout(s, cols, W, H)), rgb, nrm, ai, ni, ts, None)

    for call in (sample, pack):
        for s in (0, -1, 256, 1000):
            assert call(s=s) == -1, s
        assert b"chart size" in lib.rnb_last_error_string()
        assert call(V=-1) == -1 and call(T=-1) == -1 and call(V=2 ** 31) == -1 and call(T=2 ** 31) == -1
        assert call(verts=None) == -4 and call(tri=None) == -4
    # T n_s >= 2^31: s = 255 has 32,896 samples per triangle
    assert sample(T=65281, s=255, count=1) == -1 and b"2^31" in lib.rnb_last_error_string()
    assert pack(T=65281, s=255, cols=256, W=256 * 260, H=256 * 260) == -1
    # sample ranges: 4 triangles x 6 samples
    assert sample(first=-1) == -1 and sample(count=-1) == -1 and sample(first=1, count=24) == -1 and sample(first=25, count=0) == -1
    assert sample(first=2 ** 62, count=2 ** 62) == -1
    assert sample(pts=None) == -1 and b"every output" in lib.rnb_last_error_string()
    assert sample(count=0) == 0 and sample(first=24, count=0) == 0 and sample(T=0, count=0) == 0      # nothing is launched
    assert sample(count=0, verts=None, tri=None) == 0
    # layouts: 4 triangles = 2 cells of side 7
    assert pack(cols=1) == -1 and b"do not hold" in lib.rnb_last_error_string()       # one row of one cell
    assert pack(W=13) == -1 and pack(H=6) == -1 and pack(cols=3) == -1                  # cells reach outside the image
    assert pack(W=-1) == -1 and pack(H=-1) == -1 and pack(cols=-1) == -1
    assert pack(cols=0, W=0, H=0) == -1
    assert pack(s=1, cols=7000, W=46341, H=46341) == -1 and b"2^31" in lib.rnb_last_error_string()
    assert pack(ai=None, ni=None, ts=None) == -1 and b"every output" in lib.rnb_last_error_string()
    assert pack(rgb=None) == -4 and pack(nrm=None) == -4                                # an image without its samples
    assert lib.rnb_texture_pack(p, 8, p, 4, None, p, p, p, p, p, None) == -4
    assert pack(T=0, cols=0, W=0, H=0) == 0                                             # no texel: nothing to do


def test_python_argument_checks_fire_on_the_host():
    from tests import mesh_attrs_util as U
    mc, p, _ = U.model("tiny")
    ren = R.build_from_named_params(mc, p, torch.device("cpu"))[3]
    v = torch.zeros(3, 3, dtype=torch.float64)
    t = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    for kw in ({"chart": 0}, {"chart": 256}, {"chart": 2.5}, {"size": 0}, {"slab": 100}, {"slab": 0}, {"chunk": 65},
               {"refine": -1}, {"refine": 1}, {"refine": 1, "max_step": 0.0}):
        with pytest.raises(ValueError, match="|".join(kw)):
            ren.bake_textures(v, t, **kw)
    with pytest.raises(ValueError, match="fit"):
        ren.bake_textures(v, t, size=5)
    for bad_t in (t.long(), t[:, :2], t.numpy()):
        with pytest.raises(ValueError, match="triangles"):
            ren.bake_textures(v, bad_t)
    for bad_v in (v.float(), v[:, :2], None):
        with pytest.raises(ValueError, match="vertices"):
            ren.bake_textures(bad_v, t)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        ren.bake_textures(v, t, chart=2)
    for bad in ("yes", {"charts": 4}, {"chart": 0}, {"slab": 65}, {"to_host": False}):
        with pytest.raises(ValueError, match="bake|chart|slab"):
            ren.extract_textured_geometry(U.LO, U.HI, 8, bake=bad)


# ---- layout -------------------------------------------------------------------------------------------------------------

def _as_dict(lay):
    return lay.asdict()


@pytest.mark.parametrize("T", [0, 1, 2, 3, 80])
def test_layout_arithmetic(T):
    K = (T + 1) // 2
    for chart in (None, 1, 2, 7, 255):
        lay = R.atlas_layout(T, chart=chart)
        s = 8 if chart is None else chart
        assert _as_dict(lay) == F.layout(T, chart=chart)
        assert lay.s == s and lay.c == s + 5 and lay.samples_per_triangle == (s + 1) * (s + 2) // 2
        assert lay.cols * lay.rows >= K and (lay.cols == 0 or (lay.cols - 1) ** 2 < K <= lay.cols ** 2)
        assert (lay.rows == 0 and K == 0) or (lay.rows - 1) * lay.cols < K
        assert (lay.W, lay.H) == (lay.cols * lay.c, lay.rows * lay.c)
    for size in (64, 100, 257):
        lay = R.atlas_layout(T, size=size)
        assert _as_dict(lay) == F.layout(T, size=size)
        assert (lay.W, lay.H) == (size, size) and lay.cols == size // lay.c and lay.cols ** 2 >= K
        if lay.s < 255:       # the largest chart that fits: one more step would not
            assert (size // (lay.c + 1)) ** 2 < K
        both = R.atlas_layout(T, size=size, chart=3)
        assert both.s == 3 and both.cols == size // 8 and _as_dict(both) == F.layout(T, size=size, chart=3)


def test_layout_edges():
    assert R.atlas_layout(80, chart=2).cols == 7 and R.atlas_layout(80, chart=2).rows == 6      # 40 cells: a short last row
    assert R.atlas_layout(5, chart=1).asdict() == dict(s=1, c=6, cols=2, rows=2, W=12, H=12, samples_per_triangle=3)
    assert R.atlas_layout(80, size=64).s == 4                       # 7 x 7 cells of 9 hold 40; cells of 10 give 6 x 6 = 36
    with pytest.raises(ValueError, match="fit"):
        R.atlas_layout(80, size=41)                                 # 6 x 6 cells of side 6 hold 36 < 40
    assert R.atlas_layout(80, size=42).s == 1
    with pytest.raises(ValueError, match="fit"):
        R.atlas_layout(80, size=64, chart=5)
    for bad in ({"chart": 0}, {"chart": 256}, {"size": 0}, {"size": -4}, {"chart": True}):
        with pytest.raises(ValueError):
            R.atlas_layout(4, **bad)
    with pytest.raises(ValueError):
        R.atlas_layout(-1)
    # UVs: the corner texels' centres; both halves turn the same way
    for T, kw in ((1, {"chart": 2}), (3, {"chart": 1}), (80, {"size": 100}), (80, {"chart": 7})):
        lay = R.atlas_layout(T, **kw)
        uv = R.atlas_uv(lay, T)
        assert uv.dtype == np.float64 and uv.shape == (T, 3, 2) and np.array_equal(uv, F.uv(lay.asdict(), T))
        xy = F.corner_texels(lay.asdict(), T)
        assert np.array_equal(uv[..., 0], (xy[..., 0] + 0.5) / lay.W) and np.array_equal(uv[..., 1], 1 - (xy[..., 1] + 0.5) / lay.H)
        e1, e2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
        assert (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0] < 0).all()
    assert R.atlas_uv(R.atlas_layout(0), 0).shape == (0, 3, 2)
    with pytest.raises(ValueError, match="hold"):
        R.atlas_uv(R.atlas_layout(4, chart=2), 5)


# ---- ownership, ranks -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [1, 2, 3, 7, 8, 16])
def test_every_texel_of_a_cell_has_one_owner_and_lattice_texels_map_to_themselves(s):
    c = s + 5
    j, i = np.meshgrid(np.arange(c), np.arange(c), indexing="ij")
    up, a1, a2 = F.cell_owner(s, i, j)
    assert ((a1 >= 0) & (a2 >= 0) & (a1 + a2 <= s)).all()
    assert np.array_equal(~up, i + j <= s + 3)                       # one half or the other, never both
    # lattice texels: (1 + a1, 1 + a2) of the lower half, (c - 2 - a1, c - 2 - a2) of the upper half
    seen = {False: set(), True: set()}
    for b1 in range(s + 1):
        for b2 in range(s + 1 - b1):
            for half, (x, y) in ((False, (1 + b1, 1 + b2)), (True, (c - 2 - b1, c - 2 - b2))):
                u, g1, g2 = F.cell_owner(s, x, y)
                assert (bool(u), int(g1), int(g2)) == (half, b1, b2), (s, half, b1, b2)
                seen[half].add((x, y))
    assert not (seen[False] & seen[True]) and len(seen[False]) == len(seen[True]) == F.n_samples(s)
    # the ranks number the lattice 0 .. n_s - 1, rows of constant a2, and unrank inverts rank
    r = np.arange(F.n_samples(s))
    b1, b2 = F.unrank(s, r)
    assert np.array_equal(F.rank(s, b1, b2), r) and (b1 + b2 <= s).all() and (np.diff(b2) >= 0).all()
    assert np.array_equal(b1[b2 == 0], np.arange(s + 1)) and int(b2[-1]) == s


def _chart_points(s, rng, n):
    """points of the lower chart in cell texel-centre coordinates: n random ones, the corners, and points on the three
    edges at multiples of 1/64 (exact in binary, so px + py <= s + 2 holds as computed)"""
    w = rng.dirichlet([1.0, 1.0, 1.0], n)
    px, py = 1.0 + w[:, 1] * s, 1.0 + w[:, 2] * s
    inside = (px - 1.0) + (py - 1.0) <= s
    e = np.arange(0, 64 * s + 1) / 64.0
    ex = np.concatenate([1.0 + e, np.full_like(e, 1.0), 1.0 + e])
    ey = np.concatenate([np.full_like(e, 1.0), 1.0 + e, (1.0 + s) - e])
    return np.concatenate([px[inside], ex]), np.concatenate([py[inside], ey])


@pytest.mark.parametrize("s", [1, 2, 7])
def test_a_bilinear_lookup_reads_only_its_own_triangles_texels(s):
    rng = np.random.default_rng(100 + s)
    c = s + 5
    px, py = _chart_points(s, rng, 200000 if s < 7 else 100000)
    for half in (False, True):
        qx, qy = (px, py) if not half else ((c - 1.0) - px, (c - 1.0) - py)      # the upper chart is the lower one turned by 180
        xs, ys, ws = F.bilinear_taps(qx, qy)
        used = ws > 0
        assert (xs[used] >= 0).all() and (xs[used] < c).all() and (ys[used] >= 0).all() and (ys[used] < c).all(), "inside the cell"
        up, _, _ = F.cell_owner(s, np.clip(xs, 0, c - 1), np.clip(ys, 0, c - 1))
        assert (up[used] == half).all(), f"s = {s}: a tap with weight > 0 belongs to the other half"
    # with a cell of s + 4 the property fails: the hypotenuse's midpoint region reads the other half
    xs, ys, ws = F.bilinear_taps(px, py)
    assert ((xs + ys > s + 2) & (ws > 0)).any(), "taps on the diagonal i + j = s + 3 are needed: s + 4 would give them to both"


@pytest.mark.parametrize("T,kw", [(3, {"chart": 1}), (7, {"chart": 2}), (9, {"size": 40, "chart": 2}), (80, {"chart": 7})])
def test_the_footprint_holds_in_the_image_across_neighbouring_cells(T, kw):
    """through the image-level functions: uv corners -> lookup taps -> the owner map of the whole image"""
    lay = R.atlas_layout(T, **kw)
    L = lay.asdict()
    sample, owner = F.texel_map(L, T)
    uv = F.uv(L, T)
    rng = np.random.default_rng(T)
    n = 4000
    tri = rng.integers(0, T, n)
    bary = rng.dirichlet([1.0, 1.0, 1.0], n)
    corner = rng.integers(0, 3, 300)
    edge = rng.integers(0, 3, 600)
    tt = rng.random(600)
    eb = np.zeros((600, 3))
    eb[np.arange(600), edge] = tt
    eb[np.arange(600), (edge + 1) % 3] = 1.0 - tt
    tri = np.concatenate([tri, rng.integers(0, T, 900)])
    bary = np.concatenate([bary, np.eye(3)[corner], eb])
    uvc = uv[tri]
    u = (bary[:, 0] * uvc[:, 0, 0] + bary[:, 1] * uvc[:, 1, 0]) + bary[:, 2] * uvc[:, 2, 0]
    v = (bary[:, 0] * uvc[:, 0, 1] + bary[:, 1] * uvc[:, 1, 1]) + bary[:, 2] * uvc[:, 2, 1]
    xs, ys, ws = F.bilinear_taps(u * lay.W - 0.5, (1.0 - v) * lay.H - 0.5)
    # a tap whose weight is rounding noise of the uv arithmetic (1e-9 of a texel) is not a read of the chart
    used = ws > 1e-9
    assert (xs[used] >= 0).all() and (xs[used] < lay.W).all() and (ys[used] >= 0).all() and (ys[used] < lay.H).all()
    own = owner[np.clip(ys, 0, lay.H - 1), np.clip(xs, 0, lay.W - 1)]
    assert (own[used] == np.broadcast_to(tri[:, None], own.shape)[used]).all()
    assert (sample[np.clip(ys, 0, lay.H - 1), np.clip(xs, 0, lay.W - 1)][used] >= 0).all()
    # the texels of triangle t: its half-cell, nothing else; margins and missing triangles are empty
    n_s = lay.samples_per_triangle
    assert np.array_equal(sample >= 0, (owner >= 0) & (owner < T))
    assert np.array_equal(sample[sample >= 0] // n_s, owner[sample >= 0])
    for t in range(T):
        assert set(np.unique(sample[owner == t]) - t * n_s) == set(range(n_s)), "every lattice sample has a texel"
    # the lookup at the corners returns the corner samples
    img = np.where(sample >= 0, sample, -1).astype(np.float64)[..., None]
    got = F.lookup(img, uv, np.repeat(np.arange(T), 3), np.tile(np.eye(3), (T, 1)))[:, 0].reshape(T, 3)
    s = lay.s
    want = np.arange(T)[:, None] * n_s + np.array([F.rank(s, 0, 0), F.rank(s, s, 0), F.rank(s, 0, s)])[None]
    # ((x + 0.5) / W) W - 0.5 is x up to a few 2^-52 W, and a neighbouring tap's value differs by at most T n_s)
    assert np.abs(got - want).max() < 1e-9


def test_sample_texture_is_the_reference_lookup():
    rng = np.random.default_rng(5)
    T = 9
    lay = R.atlas_layout(T, chart=3)
    uv = R.atlas_uv(lay, T)
    img = rng.random((lay.H, lay.W, 3))
    tri = rng.integers(-1, T, 500)
    bary = rng.dirichlet([1.0, 1.0, 1.0], 500)
    bary[tri < 0] = np.nan
    got = R.sample_texture(torch.from_numpy(img), torch.from_numpy(uv), torch.from_numpy(tri), torch.from_numpy(bary)).numpy()
    want = F.lookup(img, uv, tri, bary)
    assert got.shape == (500, 3) and np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[tri < 0]).all()
    assert np.nanmax(np.abs(got - want)) < 1e-14
    u8 = (img * 255).astype(np.uint8)
    got8 = R.sample_texture(torch.from_numpy(u8[..., 0]), torch.from_numpy(uv), torch.from_numpy(tri).int(), torch.from_numpy(bary).float())
    assert got8.shape == (500,) and got8.dtype == torch.float64
    assert R.sample_texture(torch.from_numpy(img), torch.from_numpy(uv), torch.zeros(0, dtype=torch.int64), torch.zeros(0, 3)).shape == (0, 3)
    with pytest.raises(ValueError, match="uv_corners"):
        R.sample_texture(torch.from_numpy(img), torch.from_numpy(uv[:, :, 0]), torch.from_numpy(tri), torch.from_numpy(bary))


def test_reference_sample_points_have_the_stated_properties():
    from tests import mesh_raycast_ref as MR
    v, t = MR.icosphere(1)
    for s in (1, 2, 7):
        P, n_bad = F.sample_points(v, t, s)
        n_s = F.n_samples(s)
        assert P.dtype == np.float32 and P.shape == (80 * n_s, 3) and n_bad == 0
        P = P.reshape(80, n_s, 3)
        corners = [F.rank(s, 0, 0), F.rank(s, s, 0), F.rank(s, 0, s)]
        assert np.array_equal(P[:, corners], v[t].astype(np.float32))
        part, _ = F.sample_points(v, t, s, first=n_s + 1, count=2 * n_s)
        assert np.array_equal(part, P.reshape(-1, 3)[n_s + 1:3 * n_s + 1])


# ---- files ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1, 3), (1, 1, 4), (5, 7, 3), (6, 13, 4), (32, 30, 4)])
def test_png_round_trip(tmp_path, shape):
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    img[0, 0] = 255
    path = tmp_path / "a.png"
    R.write_png(path, img)
    back = R.read_png(path)
    assert back.dtype == np.uint8 and np.array_equal(back, img)
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR" and data[-8:-4] == b"IEND"
    for bad in (img.astype(np.float32), img[..., 0], img[..., :2] if shape[2] == 3 else img[:0]):
        with pytest.raises(ValueError, match="write_png"):
            R.write_png(tmp_path / "b.png", bad)
    with open(tmp_path / "c.png", "wb") as f:
        f.write(data[:40] + bytes([data[40] ^ 1]) + data[41:])
    with pytest.raises(Exception):
        R.read_png(tmp_path / "c.png")


@pytest.mark.parametrize("shape", [(1, 1, 3), (5, 7, 3), (6, 13, 4), (40, 33, 4)])
def test_png_against_pillow(tmp_path, shape):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(1 + sum(shape))
    # smooth rows and noise: Pillow then chooses several row filters
    img = (np.linspace(0, 255, shape[1])[None, :, None] * np.ones(shape)).astype(np.uint8)
    img[::2] = rng.integers(0, 256, img[::2].shape, dtype=np.uint8)
    R.write_png(tmp_path / "ours.png", img)
    with Image.open(tmp_path / "ours.png") as im:
        assert im.mode == ("RGB" if shape[2] == 3 else "RGBA") and np.array_equal(np.asarray(im), img)
    Image.fromarray(img).save(tmp_path / "theirs.png")
    assert np.array_equal(R.read_png(tmp_path / "theirs.png"), img)


def _unfilter_case(ft, rows):
    """a PNG made by hand whose rows all use row filter `ft`"""
    import struct
    import zlib
    H, stride = rows.shape
    bpp = 3
    raw = np.zeros((H, stride + 1), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.int64)
    for y in range(H):
        cur = rows[y].astype(np.int64)
        left = np.concatenate([np.zeros(bpp, dtype=np.int64), cur[:-bpp]])
        ul = np.concatenate([np.zeros(bpp, dtype=np.int64), prev[:-bpp]])
        if ft == 0:
            pred = 0
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = prev
        elif ft == 3:
            pred = (left + prev) // 2
        else:
            p = left + prev - ul
            pa, pb, pc = np.abs(p - left), np.abs(p - prev), np.abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, ul))
        raw[y, 0], raw[y, 1:] = ft, (cur - pred) & 255
        prev = cur

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", stride // bpp, H, 8, 2, 0, 0, 0))
            + chunk(b"tEXt", b"Comment\0hand made") + chunk(b"IDAT", zlib.compress(raw.tobytes())) + chunk(b"IEND", b""))


@pytest.mark.parametrize("ft", [0, 1, 2, 3, 4])
def test_read_png_undoes_every_row_filter(tmp_path, ft):
    rng = np.random.default_rng(ft)
    rows = rng.integers(0, 256, (6, 3 * 11), dtype=np.uint8)
    with open(tmp_path / "f.png", "wb") as f:
        f.write(_unfilter_case(ft, rows))
    assert np.array_equal(R.read_png(tmp_path / "f.png"), rows.reshape(6, 11, 3))


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("with_scale", [False, True])
def test_obj_round_trip(tmp_path, with_normals, with_scale):
    from tests import mesh_raycast_ref as MR
    v, t = MR.icosphere(1)
    rng = np.random.default_rng(3)
    v = v + rng.standard_normal(v.shape) * 1e-3
    lay = R.atlas_layout(len(t), chart=2)
    uv = R.atlas_uv(lay, len(t))
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32) if with_normals else None
    scale = np.diag([2.5, 2.5, 2.5, 1.0]) if with_scale else None
    if with_scale:
        scale[:3, 3] = [0.1, -0.2, 0.3]
    path = tmp_path / "mesh.obj"
    material = {"albedo": "mesh_albedo.png", "normal": "mesh_normal.png"}
    R.write_obj(path, v, t, uv, normals=nrm, scale_mat=scale, material=material)
    m = R.read_obj(path)
    want_v = v * 2.5 + np.array([0.1, -0.2, 0.3])[None] if with_scale else v
    assert m["vertices"].dtype == np.float64 and np.array_equal(m["vertices"], want_v)
    assert m["triangles"].dtype == np.int32 and np.array_equal(m["triangles"], t)
    assert np.array_equal(m["uv"], uv)
    assert (m["normals"] is None) if not with_normals else np.array_equal(m["normals"], nrm)
    assert m["material"] == material
    mtl = open(tmp_path / "mesh.mtl").read()
    assert "newmtl baked" in mtl and "map_Kd mesh_albedo.png" in mtl and "norm mesh_normal.png" in mtl
    text = open(path).read()
    assert "mtllib mesh.mtl" in text and text.count("\nvt ") == 3 * len(t) and text.count("\nf ") == len(t)
    # without a material no MTL is named; an empty mesh round-trips
    R.write_obj(tmp_path / "plain.obj", v, t, uv)
    assert R.read_obj(tmp_path / "plain.obj")["material"] is None and not os.path.exists(tmp_path / "plain.mtl")
    R.write_obj(tmp_path / "empty.obj", np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32), np.zeros((0, 3, 2)))
    e = R.read_obj(tmp_path / "empty.obj")
    assert e["vertices"].shape == (0, 3) and e["triangles"].shape == (0, 3) and e["uv"].shape == (0, 3, 2)
    with pytest.raises(ValueError, match="uv"):
        R.write_obj(tmp_path / "x.obj", v, t, uv[:-1])
    with pytest.raises(ValueError, match="outside"):
        R.write_obj(tmp_path / "x.obj", v[:5], t, uv)
