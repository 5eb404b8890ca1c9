"""The grid, mesh, ray-generation and whole-image entry points between guard bands (tests/guard_bands.py).

The rule of tests/test_gpu_guard_render.py: every call runs once on ordinary allocations and once under guarded() with its
inputs passed through guard(); both bands of every allocation must still hold their pattern, the registry must have seen the
buffers the call is known to make (a workspace of exactly the query that applies, every output whose size the call fixes or
a scan decides), and every result must equal the unguarded run bit for bit.  All of these calls are reproducible (integer
atomics only: include/rnbneus.h), so nothing here is held to less than bit equality.  No fp64 oracle is involved; the small
inputs are those of each feature's own GPU test, from the helper modules those tests use.
Every case prints one line starting with GUARD."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests import guard_bands as GB
from tests import mesh_attrs_util as U
from tests import mesh_components_ref as MC
from tests import mesh_distance_ref as MD
from tests import mesh_large_shapes as ML
from tests import mesh_raycast_ref as MR
from tests import mesh_simplify_ref as MS
from tests import source_maps_util
from tests.golden_util import GOLDEN_DIR, Golden, load_raygen
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device
from tests.mc_shapes import sphere

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
    print(f"GUARD geometry {tag}: {len(s.registry)} guarded allocations, {time.perf_counter() - t0:.2f} s")
    return s, got


def _query(R, name, *args):
    b = C.c_int64()
    R.native.check(getattr(R.native.load(), name)(*args, C.byref(b)))
    return b.value


def _made(s, what, **kw):
    got = [e for e in s.seen(**kw) if e.how != "guard"]
    assert got, f"{what}: no guarded allocation of {kw}"
    return got


# ------------------------------------------------------------------------------------------------------------- the SDF grid
def _grid_desc(R, res, x0, x1, lo=U.LO, hi=U.HI):
    gd = R.native.GridDesc()
    for d in range(3):
        gd.bound_min[d], gd.bound_max[d] = float(lo[d]), float(hi[d])
    gd.resolution, gd.x_begin, gd.x_end, gd.out_scale = res, x0, x1, -1.0
    return gd


@pytest.mark.parametrize("which", ["sharp", "tiny"])
def test_extract_fields(R, which):
    """resolution 20 (8,000 points: 64 rows short of the pad) with the reference's chunk keyword"""
    ren = U.renderer(R, which, device())
    s, _ = _twice(f"extract_fields {which}", lambda x: ren.extract_fields(U.LO, U.HI, 20, chunk=8, to_host=False), {})
    ws = _query(R, "rnb_sdf_grid_workspace_bytes", C.byref(ren.desc), C.byref(_grid_desc(R, 20, 0, 20)))
    _made(s, "rnb_sdf_grid workspace", nbytes=max(ws, 256), dtype=u8)
    _made(s, "volume", shape=(20, 20, 20), dtype=torch.float32)


def test_extract_fields_sharded_with_one_rank(R, tmp_path):
    """the data-parallel form on a group of one rank (its slab is the volume), and one x-slab of a grid through rnb_sdf_grid,
    as a rank of a larger group would evaluate it"""
    ren = U.renderer(R, "sharp", device())
    lib = R.native.load()
    own = not dist.is_initialized()
    if own:
        dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'store'}", rank=0, world_size=1)
    try:
        group = dist.group.WORLD
        assert dist.get_world_size(group) == 1
        s, got = _twice("extract_fields group of one", lambda x: ren.extract_fields(U.LO, U.HI, 20, chunk=8, group=group, to_host=False), {})
        _made(s, "slab", shape=(20, 20, 20), dtype=torch.float32)
    finally:
        if own:
            dist.destroy_process_group()
    plain = ren.extract_fields(U.LO, U.HI, 20, to_host=False)
    assert torch.equal(plain, got), "a group of one evaluates the whole volume"
    res, x0, x1 = 37, 5, 30
    gd = _grid_desc(R, res, x0, x1)
    ws_bytes = max(_query(R, "rnb_sdf_grid_workspace_bytes", C.byref(ren.desc), C.byref(gd)), 256)

    def slab(x):
        packed = ren._pack(False)
        vol = torch.full((x1 - x0, res, res), float("nan"), dtype=torch.float32, device=device())
        ws = torch.empty(ws_bytes, dtype=u8, device=device())
        with R.native.on_device(vol) as stream:
            R.native.check(lib.rnb_sdf_grid(C.byref(ren.desc), R.native.ptr(packed), C.byref(gd), R.native.ptr(vol),
                                            R.native.ptr(ws), ws.numel(), stream))
        return vol

    s, vol = _twice("rnb_sdf_grid x-slab 5..30 of 37", slab, {})
    assert bool(torch.isfinite(vol).all()), "every sample of the slab is written"
    _made(s, "slab workspace", nbytes=ws_bytes, dtype=u8)


@pytest.mark.parametrize("brick", [4, 8])
def test_extract_fields_sparse(R, brick):
    """resolution 33: 32 cells per edge, whole bricks; the brick lists, the mask and the volume are sized from counters"""
    ren = U.renderer(R, "sharp", device())

    def call(x):
        u, info = ren.extract_fields_sparse(U.LO, U.HI, 33, brick=brick)
        return u, info

    s, (u, info) = _twice(f"extract_fields_sparse brick {brick}", call, {})
    assert 0 < info["bricks_active"] < info["bricks_total"], info
    sd = R.native.SparseGridDesc(brick, 0.0, 1.0)
    ws = _query(R, "rnb_sdf_grid_sparse_workspace_bytes", C.byref(ren.desc), C.byref(_grid_desc(R, 33, 0, 33)), C.byref(sd))
    _made(s, "sparse workspace", nbytes=max(ws, 256), dtype=u8)
    nb = R.native.brick_geometry(33, brick)["nb"]
    _made(s, "volume", shape=(33, 33, 33), dtype=torch.float32)
    _made(s, "brick mask", shape=(nb, nb, nb), dtype=u8)


# ------------------------------------------------------------------------------------------------------- marching cubes
MC_VOLUMES = {"noise_0": (MC.noise_volume, 0.0), "noise_0.37": (MC.noise_volume, 0.37),
              "constant": (lambda: np.full((5, 6, 7), 1.0, dtype=np.float32), 0.0),
              "sphere_40": (lambda: -sphere(40), 0.0)}


@pytest.mark.parametrize("name", list(MC_VOLUMES))
def test_marching_cubes(R, name):
    """the (37, 21, 50) noise volume (every case, ragged tiles) at both thresholds, a constant volume (empty outputs), a sphere:
    the vertex and triangle arrays are sized by the count pass's scan"""
    make, thr = MC_VOLUMES[name]
    u = make()
    s, (v, t) = _twice(f"marching_cubes {name}", lambda x: R.marching_cubes(x["u"], thr), {"u": u})
    _made(s, "workspace", nbytes=_query(R, "rnb_marching_cubes_workspace_bytes", *u.shape), dtype=u8)
    if name == "constant":
        assert v.shape == (0, 3) and t.shape == (0, 3)
    else:
        assert v.shape[0] > 100 and t.shape[0] > 100
        _made(s, "vertices", shape=tuple(v.shape), dtype=torch.float64)
        _made(s, "triangles", shape=tuple(t.shape), dtype=torch.int32)


_MESH = {}


def _mc_mesh(R, name):
    """the device marching cubes of the cleanup tests' volumes (tests/mesh_components_ref.py), as numpy"""
    if name not in _MESH:
        u = {"A": MC.volume_a, "noise": MC.noise_volume}[name]()
        v, t = R.marching_cubes(_dev(u), 0.0)
        _MESH[name] = (v.cpu().numpy(), t.cpu().numpy())
    return _MESH[name]


# ---------------------------------------------------------------------------------------------------- vertex attributes
@pytest.mark.parametrize("which,V,chunk", [("sharp", 200, 64), ("sharp", 1, 64), ("tiny", 65, 64), ("sharp_bf16", 200, 128)])
def test_vertex_attributes(R, which, V, chunk):
    """V no multiple of the chunk: the last chunk is ragged, and one workspace of the chunk's size serves every chunk"""
    ren = U.renderer(R, which, device())
    s, out = _twice(f"vertex_attributes {which} V={V} chunk={chunk}", lambda x: ren.vertex_attributes(x["pts"], chunk=chunk),
                    {"pts": U.point_batch(which, V)})
    for k, width, dt in (("points", 3, torch.float32), ("sdf", 1, torch.float32), ("gradient", 3, torch.float32),
                         ("normal", 3, torch.float32), ("albedo", ren.desc.col_d_out, torch.float32), ("rgb", 3, u8)):
        assert tuple(out[k].shape) == (V, width)
        _made(s, k, shape=(V, width), dtype=dt)
    assert [e for e in s.seen(dtype=u8) if "mesh_vertex_attrs" in e.site and e.nbytes > 3 * V], "the workspace was not guarded"


def test_vertex_attributes_with_a_newton_step(R):
    ren = U.renderer(R, "sharp", device())
    _twice("vertex_attributes refine=1", lambda x: ren.vertex_attributes(x["pts"], refine=1, max_step=0.05, chunk=128),
           {"pts": U.point_batch("sharp", 200)})


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_extract_textured_geometry(R, sparse):
    """grid, marching cubes and the per-vertex attributes in one call (resolution 24: a few hundred vertices)"""
    ren = U.renderer(R, "sharp", device())
    kw = dict(sparse=True, brick=8) if sparse else {}
    s, tex = _twice(f"extract_textured_geometry sparse={sparse}",
                    lambda x: ren.extract_textured_geometry(U.LO, U.HI, 24, to_host=False, **kw), {})
    V = tex["vertices"].shape[0]
    assert V > 100
    _made(s, "vertices", shape=(V, 3), dtype=torch.float64)
    _made(s, "colors", shape=(V, 3), dtype=u8)


# ------------------------------------------------------------------------------------------------------------ mesh cleanup
def test_clean_mesh_on_the_noise_mesh(R):
    """the noise volume's mesh: hundreds of components; labels, per-component statistics and the compacted arrays (sized by a scan)"""
    v, t = _mc_mesh(R, "noise")

    def call(x):
        comp = R.mesh_components(x["t"], vertices=x["v"])
        return comp, R.clean_mesh(x["v"], x["t"], keep_largest=3), R.clean_mesh(x["v"], x["t"], min_fraction=0.01, by="triangles")

    s, (comp, kept, frac) = _twice("clean_mesh noise", call, {"v": v, "t": t})
    assert comp["n_components"] > 50
    _made(s, "workspace", nbytes=_query(R, "rnb_mesh_clean_workspace_bytes", len(v), len(t)), dtype=u8)
    _made(s, "labels", shape=(len(v),), dtype=torch.int32)
    _made(s, "compacted triangles", shape=tuple(kept["triangles"].shape), dtype=torch.int32)
    _made(s, "compacted vertices", shape=tuple(kept["vertices"].shape), dtype=torch.float64)
    assert 0 < kept["triangles"].shape[0] < len(t)


def test_clean_mesh_small_meshes(R):
    for name, make in MC.SMALL_MESHES.items():
        v, t = make() if callable(make) else make
        v, t = np.asarray(v, dtype=np.float64).reshape(-1, 3), np.asarray(t, dtype=np.int32).reshape(-1, 3)
        _twice(f"clean_mesh {name}", lambda x: (R.mesh_components(x["t"], vertices=x["v"]), R.clean_mesh(x["v"], x["t"], keep_largest=1)),
               {"v": v, "t": t})


def test_clean_mesh_past_the_first_chunk_of_the_block_sum_scans(R):
    """PREFIX of tests/mesh_large_shapes.py: 1,027 vertex tile sums (the root-rank scan and the vertex half of the compaction
    scan store through a second chunk) and 489 triangle tile sums, all carved from the one workspace"""
    d = ML.big("PREFIX")
    v, t, n_loose = d["vertices"], d["triangles"], d["n_loose"]
    assert ML.tiles(len(v)) == 1027 and ML.tiles(len(t)) == 489 and ML.chunks(len(v)) == 2 and ML.chunks(len(t)) == 1
    s, out = _twice("clean_mesh PREFIX", lambda x: R.clean_mesh(x["v"], x["t"]), {"v": v, "t": t})
    assert out["info"]["n_vertices"] == (len(v), len(v) - n_loose) and int(out["vertex_index"][0]) == n_loose
    _made(s, "workspace", nbytes=_query(R, "rnb_mesh_clean_workspace_bytes", len(v), len(t)), dtype=u8)
    _made(s, "labels", shape=(len(v),), dtype=torch.int32)
    _made(s, "compacted vertices", shape=(len(v) - n_loose, 3), dtype=torch.float64)
    _made(s, "vertex_index", shape=(len(v) - n_loose,), dtype=torch.int64)


# ---------------------------------------------------------------------------------------------------------- simplification
@pytest.mark.parametrize("double", [False, True])
def test_simplify_mesh_hub(R, double):
    """4,096 fan triangles round one vertex: every insertion of the cluster table meets the hub's slot"""
    v, t = MS.hub(double)
    attrs = np.arange(len(v), dtype=np.float32)
    s, out = _twice(f"simplify_mesh hub double={double}",
                    lambda x: R.simplify_mesh(x["v"], x["t"], cell_size=1.0, origin=(0.0, 0.0, 0.0), attributes={"id": x["a"]}),
                    {"v": v, "t": t, "a": attrs})
    assert out["triangles"].shape[0] == 4096
    _made(s, "workspace", nbytes=_query(R, "rnb_mesh_simplify_workspace_bytes", len(v), len(t)), dtype=u8)
    _made(s, "vertex_cluster", shape=(len(v),), dtype=torch.int32)
    _made(s, "triangles", shape=(4096, 3), dtype=torch.int32)
    _made(s, "triangle_index", shape=(4096,), dtype=torch.int64)


@pytest.mark.parametrize("n", [300, 3703])
def test_simplify_mesh_target_triangles(R, n):
    """the search over resolutions: one count per resolution tried in ONE workspace, then the emit"""
    v, t = _mc_mesh(R, "A")
    s, out = _twice(f"simplify_mesh target {n}", lambda x: R.simplify_mesh(x["v"], x["t"], target_triangles=n), {"v": v, "t": t})
    assert 0 < out["triangles"].shape[0] <= n and len(out["info"]["tried"]) >= 1
    _made(s, "workspace", nbytes=_query(R, "rnb_mesh_simplify_workspace_bytes", len(v), len(t)), dtype=u8)
    _made(s, "triangles", shape=tuple(out["triangles"].shape), dtype=torch.int32)


@pytest.mark.parametrize("h", [1.5, 4.0])
def test_simplify_mesh_noise(R, h):
    v, t = _mc_mesh(R, "noise")
    _twice(f"simplify_mesh noise h={h}", lambda x: R.simplify_mesh(x["v"], x["t"], cell_size=h), {"v": v, "t": t})


# --------------------------------------------------------------------------------------------------------- mesh evaluation
def _index_state(index):
    """what a MeshIndex holds that does not depend on the order of its bin entries (integer atomics on per-cell cursors)"""
    return dict(dims=list(index.dims), n_entries=index.n_entries, n_cells=index.n_cells, cell_start=index.cell_start,
                entries_sorted=torch.sort(index.entries).values, corners=index.corners)


def test_closest_points_on_the_torus(R):
    case = MD.torus_case()
    q = np.concatenate([case["queries"], case["far"]])

    def call(x):
        out = {}
        for cells in (None, 1, (7, 3, 5)):
            index = R.MeshIndex(x["v"], x["t"], cells=cells)
            out[str(cells)] = (index.closest(x["q"]), _index_state(index))
        return out

    s, out = _twice("MeshIndex.closest torus", call, {"v": case["vertices"], "t": case["triangles"], "q": q})
    index = R.MeshIndex(_dev(case["vertices"]), _dev(case["triangles"]))
    _made(s, "bins workspace", nbytes=_query(R, "rnb_mesh_bins_workspace_bytes", index.n_cells), dtype=u8)
    _made(s, "cell_start", shape=(index.n_cells + 1,), dtype=torch.int64)
    _made(s, "entries", shape=(index.n_entries,), dtype=torch.int32)
    _made(s, "corners", shape=(1200, 9), dtype=torch.float64)
    _made(s, "dist2", shape=(len(q),), dtype=torch.float64)


def test_the_spread_mesh_crosses_scan_tiles(R):
    """2,500 separate triangles (three scan tiles) whose areas span 10^6: the area scan, the samples, the bins"""
    v, t, zero = MD.spread_mesh()

    def call(x):
        samples = R.sample_surface(x["v"], x["t"], 6000, seed=3)
        index = R.MeshIndex(x["v"], x["t"])
        return samples, index.closest(samples["points"][:500]), R.sample_surface(x["v"], x["t"], 1, seed=9)

    s, _ = _twice("spread mesh", call, {"v": v, "t": t})
    _made(s, "sample workspace", nbytes=_query(R, "rnb_mesh_sample_workspace_bytes", len(t)), dtype=u8)
    _made(s, "cum_area", shape=(len(t),), dtype=torch.float64)
    _made(s, "points", shape=(6000, 3), dtype=torch.float64)
    _made(s, "triangle", shape=(6000,), dtype=torch.int32)


def test_sample_surface_past_the_first_chunk_of_the_area_scan(R):
    """ISOLATED of tests/mesh_large_shapes.py: 1,029 fp64 tile sums in the sample workspace, the last five of them written
    on the second trip of the one workgroup that chains them"""
    d = ML.big("ISOLATED")
    v, t = d["vertices"], d["triangles"]
    assert ML.tiles(len(t)) == 1029 and ML.chunks(len(t)) == 2
    s, out = _twice("sample_surface ISOLATED", lambda x: R.sample_surface(x["v"], x["t"], 4096, seed=3), {"v": v, "t": t})
    assert int(out["triangle"].max()) >= ML.LINE, "a sample past triangle 2^20"
    _made(s, "sample workspace", nbytes=_query(R, "rnb_mesh_sample_workspace_bytes", len(t)), dtype=u8)
    _made(s, "cum_area", shape=(len(t),), dtype=torch.float64)
    _made(s, "points", shape=(4096, 3), dtype=torch.float64)
    _made(s, "triangle", shape=(4096,), dtype=torch.int32)


def test_sample_surface_and_mesh_distance_on_the_torus(R):
    case = MD.torus_case()
    v, t = case["vertices"], case["triangles"]
    va, ta = _mc_mesh(R, "A")

    def call(x):
        return (R.sample_surface(x["v"], x["t"], 777, seed=3),
                R.mesh_distance(x["v"], x["t"], x["v"], x["t"], n_samples=1000, thresholds=(1e-6,), return_samples=True),
                R.mesh_distance(x["va"], x["ta"], x["v"], x["t"], n_samples=2000, thresholds=(0.05, 0.2), seed=1, return_samples=True))

    s, _ = _twice("sample_surface + mesh_distance", call, {"v": v, "t": t, "va": va, "ta": ta})
    _made(s, "sample workspace", nbytes=_query(R, "rnb_mesh_sample_workspace_bytes", len(t)), dtype=u8)
    _made(s, "samples", shape=(2000, 3), dtype=torch.float64)


# ------------------------------------------------------------------------------------------------------------ ray casting
def test_mesh_raycast_first_hits(R):
    case = MR.torus_rays()
    ins = {k: case[k] for k in ("vertices", "triangles", "origins", "directions", "t_min", "t_max")}

    def call(x):
        index = R.MeshIndex(x["vertices"], x["triangles"])
        o32, d32 = x["origins"].float(), x["directions"].float()
        return (index.raycast(x["origins"], x["directions"], x["t_min"], x["t_max"]), index.raycast(o32, d32),
                index.raycast(x["origins"][:7], x["directions"][:7], 0.25, 0.9), index.raycast(x["origins"][:1], x["directions"][:1]))

    s, out = _twice("MeshIndex.raycast torus", call, ins)
    N = len(case["origins"])
    assert int(out[0]["hit"].sum()) > 100
    for what, shape, dt in (("t", (N,), torch.float64), ("triangle", (N,), torch.int32), ("bary", (N, 3), torch.float64)):
        _made(s, what, shape=shape, dtype=dt)


def test_mesh_view_maps(R):
    v, t = MR.icosphere(2)
    H, W = 12, 16
    o, d = MR.pinhole_rays(H, W, eye=(2.4, -1.1, 0.9), look_at=(0.1, 0.0, 0.05), fov_deg=50.0)
    albedo = np.random.default_rng(2).uniform(0.0, 1.0, (len(v), 3))

    def call(x):
        index = R.MeshIndex(x["v"], x["t"])
        return R.mesh_view_maps(index, x["o"], x["d"], shape=(H, W), vertex_normals=x["v"], vertex_albedo=x["albedo"])

    s, maps = _twice("mesh_view_maps icosphere", call, {"v": np.asarray(v, dtype=np.float64), "t": np.asarray(t, dtype=np.int32),
                                                          "o": o, "d": d, "albedo": albedo})
    assert 20 < int(maps["mask"].sum()) < H * W - 20, "the view holds the silhouette"
    _made(s, "t", shape=(H * W,), dtype=torch.float64)


# ----------------------------------------------------------------------------------------------------------- ray generation
def _ray_stacks(front, targets):
    """the fixture that drives one of the ray kernel's four instantiations (tests/test_gpu_raygen.py)"""
    if targets == "maps":
        return "maps", source_maps_util.load_fixture()
    if front == "list":
        return "stack", load_raygen()[0]
    z = np.load(os.path.join(GOLDEN_DIR, "image_rays_small.npz"), allow_pickle=False)
    return "stack", {k: torch.from_numpy(z[k]) for k in z.files}


def _device_rays(R, kind, fx, g):
    if kind == "maps":
        dr = R.DeviceRays.from_source_maps(fx["normals_u8"], fx["albedo_u8"], fx["masks_u8"], torch.from_numpy(fx["intrinsics_inv"]),
                                           torch.from_numpy(fx["pose"]), "cuda:0")
    else:
        dr = R.DeviceRays(fx["images"], fx["images_warmup"], fx["masks"], fx["light_directions"], fx["light_directions_warmup"],
                          fx["intrinsics_all_inv"], fx["pose_all"], "cuda:0")
    n = 0
    for k, v in list(vars(dr).items()):        # the stacks the kernel gathers from, between bands as well
        if isinstance(v, torch.Tensor) and v.is_cuda and v.is_contiguous() and v.numel():
            setattr(dr, k, g(v))
            n += 1
    assert n >= 3, f"DeviceRays holds {n} device tensors: the stacks were not found"
    return dr


@pytest.mark.parametrize("targets", ["stack", "maps"])
@pytest.mark.parametrize("front", ["list", "grid"])
def test_ray_generation(R, front, targets):
    """pixel list or grid range, stack gathers or source maps: B = 1 and B = 257 (a second workgroup with one live lane); a whole
    view, a range that starts and ends inside a row with one light and with all, a pose-only call"""
    kind, fx = _ray_stacks(front, targets)

    def call(g):
        dr = _device_rays(R, kind, fx, g)
        out = []
        if front == "list":
            for v, B in ((0, 1), (2, 257)):
                gen = torch.Generator().manual_seed(5 + B)
                px, py = torch.randint(0, dr.W, (B,), generator=gen), torch.randint(0, dr.H, (B,), generator=gen)
                for warmup in (False, True):
                    out.append(dr.sample(v, B, warmup=warmup, pixels_x=px, pixels_y=py))
            return out
        Wl = dr.W // 2
        first, count = Wl + 2, 2 * Wl + 1
        for v, kw in [(1, dict(resolution_level=1)), (0, dict(resolution_level=2, first=first, count=count, light=1)),
                      (2, dict(resolution_level=2, first=first, count=count))]:
            out.append(dr.view_rays(v, **kw))
        out.append(dr.view_rays(pose=dr.pose_between(0, 2, 0.3), resolution_level=2))
        return out

    t0 = time.perf_counter()
    tag = f"ray generation {front} {targets}"
    clean = call(lambda t: t)
    torch.cuda.synchronize()
    with GB.guarded() as s:
        got = call(GB.guard)
        torch.cuda.synchronize()
        GB.assert_intact(tag)
    GB.assert_same(tag, clean, got)
    n_rays = got[-1 if front == "grid" else 1]["rays_d"].shape[0]
    _made(s, "rays + mask [n, 7]", shape=(n_rays, 7), dtype=torch.float32)
    _made(s, "near / far", shape=(n_rays, 1), dtype=torch.float32)
    print(f"GUARD geometry {tag}: {len(s.registry)} guarded allocations, {time.perf_counter() - t0:.2f} s")


# -------------------------------------------------------------------------------------------------------- whole-image render
@pytest.mark.parametrize("chunk", [64, 48])
def test_render_image_on_a_ragged_last_chunk(R, chunk):
    """view 1 of the image fixture, 176 rays: chunks of 64 leave a last chunk of 48 rays, chunks of 48 one of 32 - each
    writes its rows into the preallocated images through ONE workspace sized for a full chunk"""
    z = np.load(os.path.join(GOLDEN_DIR, "image_rays_small.npz"), allow_pickle=False)
    fx = {k: torch.from_numpy(z[k]) for k in z.files}
    g = Golden("tiny_main_sharp")
    ren = R.build_from_named_params(g.mc, g.params(), "cuda:0")[3]

    def call(gd):
        dr = _device_rays(R, "stack", fx, gd)
        return (ren.render_image(dr, 1, api="render_rnb", perturb_overwrite=0, cos_anneal_ratio=1.0, chunk_rays=chunk, return_z_vals=True),
                ren.render_image(dr, pose=dr.pose_between(0, 2, 0.3), resolution_level=2, perturb_overwrite=0, chunk_rays=16))

    t0 = time.perf_counter()
    tag = f"render_image chunk_rays={chunk}"
    clean = call(lambda t: t)
    torch.cuda.synchronize()
    with GB.guarded() as s:
        got = call(GB.guard)
        torch.cuda.synchronize()
        GB.assert_intact(tag)
    GB.assert_same(tag, clean, got)
    N = got[0]["z_vals"].shape[0]
    assert N % chunk != 0, "the last chunk must be ragged"
    S = ren.n_samples + ren.n_importance
    flags = R.native.MODE_MVPS | R.native.FLAG_FORWARD_ONLY
    ws = _query(R, "rnb_render_workspace_bytes", C.byref(ren.desc), chunk, S, flags)
    assert [e for e in s.seen(dtype=u8) if e.nbytes >= max(ws, 256) and "_maps_begin" in e.site], \
        f"no guarded map workspace of at least rnb_render_workspace_bytes = {ws}: {[e.describe() for e in s.seen(dtype=u8)]}"
    _made(s, "z_vals", shape=(N, S), dtype=torch.float32)
    print(f"GUARD geometry {tag}: {len(s.registry)} guarded allocations, {time.perf_counter() - t0:.2f} s")
