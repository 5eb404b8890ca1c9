"""Per-vertex mesh attributes on the device (`rnb_mesh_vertex_attrs`, `NeuSRenderer.vertex_attributes`,
`extract_textured_geometry`) against the CPU oracle's `sdf_forward` / `sdf_gradient` / `color_forward` — the reference's
`sdf_network(v)`, `sdf_network.gradient(v)`, `color_network(v, g, g, feat)` (exp_runner.py:607-610) — run in fp32 and fp64
on the device's own fp32 points.

Bounds.  fp32 routes: `tests/parity.check_value` (K_OUT x the fp32 oracle's own distance from fp64 + the floor); nothing
hand-set.  Exact properties (coordinates, colour quantisation, chunking, determinism): bit equality.  The unit normal: 5e-7
absolute = 4 fp32 ulps of a component of a unit vector, against gradient / |gradient| recomputed on the host in fp32.
bf16 route: the project's stated point-wise bf16 bounds against the FP32 oracle, copied from tests/test_gpu_bf16.py
(SDF_ATOL, NRM_ATOL, OUT_ATOL = 1e-2, 1e-1, 3e-2).
Models, point batches and references: tests/mesh_attrs_util.py (computed once, shared)."""
import numpy as np
import pytest
import torch

from oracle import rnb_oracle as O
from tests import mesh_attrs_util as U
from tests import parity as P
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device

pytestmark = pytest.mark.gpu

LO, HI = U.LO, U.HI
SDF_ATOL, NRM_ATOL, OUT_ATOL = 1e-2, 1e-1, 3e-2      # tests/test_gpu_bf16.py: bf16 point-wise SDF, normal, outputs
NORMAL_ATOL = 5e-7
KEYS = ("sdf", "gradient", "albedo")


def _check_parity(tag, out, ref, keys=KEYS):
    for k in keys:
        r64, r32 = ref[k]
        e_dev, e_ref, bound = P.value_errors(out[k].cpu(), r64, r32)
        print(f"{tag}: {k} |dev - fp64| {e_dev:.3e}, fp32 oracle {e_ref:.3e}, bound {bound:.3e}")
    for k in keys:
        P.check_value(f"{tag}: {k}", out[k].cpu(), *ref[k])


def _check_epilogue(out):
    """what the epilogue kernel derives, recomputed on the host in fp32 from the device's own gradient and albedo"""
    g = out["gradient"].cpu()
    n = out["normal"].cpu()
    assert float((n - g / g.norm(dim=1, keepdim=True)).abs().max()) <= NORMAL_ATOL
    if "albedo" in out:
        assert out["rgb"].dtype == torch.uint8 and torch.equal(out["rgb"].cpu(), U.quantize_rgb(out["albedo"]))


@pytest.mark.parametrize("chunk", [64, 128])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("which", ["sharp", "tiny"])
def test_point_batches_match_the_oracle(R, which, V, chunk):
    ren = U.renderer(R, which, device())
    pts = U.point_batch(which, V)
    out = ren.vertex_attributes(pts.to(device()), chunk=chunk)
    torch.cuda.synchronize()
    assert set(out) == {"points", "sdf", "gradient", "normal", "albedo", "rgb"}
    assert torch.equal(out["points"].cpu(), pts), "points are the input, bit for bit"
    _check_parity(f"{which} V={V} chunk={chunk}", out, U.oracle_attributes(which, pts, tag=V))
    _check_epilogue(out)


@pytest.mark.parametrize("which", ["sharp", "tiny"])
def test_chunking_does_not_change_a_bit(R, which):
    """A vertex's attributes do not depend on the chunk it falls into (chunks are whole 64-vertex tiles, so the tiles are
    the same whatever the chunk), and the same call twice gives the same bits."""
    ren = U.renderer(R, which, device())
    pts = U.point_batch(which, 200).to(device())
    a = ren.vertex_attributes(pts, chunk=64)
    b = ren.vertex_attributes(pts, chunk=256)
    c = ren.vertex_attributes(pts, chunk=64)
    for k in a:
        assert torch.equal(a[k], c[k]), f"{k}: two identical calls differ"
        assert torch.equal(a[k], b[k]), f"{k}: chunk=64 and chunk=256 differ"
    x = (a["rgb"].cpu().float() / 255.0)
    assert float(x.std()) > 1e-3, "degenerate colours: the quantisation check would pass for a constant"


@pytest.mark.parametrize("res", [70, 97])
def test_grid_vertices_become_the_hosts_fp32_points(R, res):
    ren = U.renderer(R, "sharp", device())
    u = ren.extract_fields(LO, HI, res, to_host=False)
    v, t = R.marching_cubes(u, 0.0)
    assert v.shape[0] > 1000 and v.dtype == torch.float64
    out = ren.vertex_attributes(grid_vertices=v, bounds=(LO, HI), resolution=res, chunk=4096)   # several chunks
    want = U.host_points(v.cpu().numpy(), res)
    assert torch.equal(out["points"].cpu(), want)
    # the same vertices as fp32 points give the same attributes
    again = ren.vertex_attributes(want.to(device()), chunk=4096)
    for k in out:
        assert torch.equal(out[k], again[k]), k
    _check_epilogue(out)


@pytest.mark.parametrize("which", ["sharp", "tiny"])
def test_one_newton_step_matches_the_oracle(R, which):
    ren = U.renderer(R, which, device())
    pts = U.point_batch(which, 200)
    # 0.05: the uniform half is clamped, the near-surface half (within 0.02) mostly is not
    out = ren.vertex_attributes(pts.to(device()), refine=1, max_step=0.05, chunk=128)
    r64, r32 = U.oracle_newton(which, pts, 0.0, 0.05)
    moved = (r64 - pts.double()).norm(dim=1)
    assert int((moved < 0.049).sum()) >= 50 and int((moved > 0.0499).sum()) >= 50, "both branches of the clamp must run"
    e_dev, e_ref, bound = P.value_errors(out["points"].cpu(), r64, r32)
    print(f"{which}: one Newton step |dev - fp64| {e_dev:.3e}, fp32 oracle {e_ref:.3e}, bound {bound:.3e}")
    P.check_value(f"{which}: points after one Newton step", out["points"].cpu(), r64, r32)
    # the attributes are those of the moved points
    _check_parity(f"{which} refined", out, U.oracle_attributes(which, out["points"].cpu()))
    _check_epilogue(out)
    # a threshold moves the target level: sdf = -threshold
    lev = ren.vertex_attributes(pts.to(device()), refine=1, max_step=0.05, threshold=0.03, chunk=128)
    r64, r32 = U.oracle_newton(which, pts, -0.03, 0.05)
    P.check_value(f"{which}: one Newton step towards sdf = -0.03", lev["points"].cpu(), r64, r32)
    # max_step bounds every displacement
    tight = ren.vertex_attributes(pts.to(device()), refine=1, max_step=1e-4, chunk=128)
    d = (tight["points"].cpu().double() - pts.double()).norm(dim=1)
    print(f"{which}: max displacement at max_step 1e-4: {float(d.max()):.12e}; moved {int((d > 0).sum())} of {len(d)}")
    assert float(d.max()) <= 1e-4 * (1 + 1e-6)
    assert float(d.max()) > 0.99e-4 and int((d > 0.5e-4).sum()) > 150, "the step is clamped, not dropped"


def _check_textured(R, ren, tex, res, sparse):
    vg, tg = ren.extract_geometry(LO, HI, res, threshold=0.0, backend="native", sparse=sparse, brick=8 if sparse else None)
    assert tex["vertices"].dtype == np.float64 and tex["triangles"].dtype == np.int32
    assert np.array_equal(tex["vertices"], vg) and np.array_equal(tex["triangles"], tg)
    V = vg.shape[0]
    assert V > 1000 and tex["normals"].shape == (V, 3) and tex["colors"].shape == (V, 3) and tex["colors"].dtype == np.uint8
    pts = torch.tensor(tex["vertices"]).type(torch.float32)
    out = {"sdf": torch.from_numpy(tex["sdf"]), "albedo": torch.from_numpy(tex["albedo"])}
    ref = U.oracle_attributes("sharp", pts, tag=("textured", res))
    _check_parity(f"textured res {res} sparse={sparse}", out, ref, keys=("sdf", "albedo"))
    # normals: the oracle's unit gradient (bound of the gradient rule, scaled by 1 / |g|: normalising divides the error)
    g64, g32 = ref["gradient"]
    n64, n32 = (torch.nn.functional.normalize(g, dim=1) for g in (g64, g32))
    P.check_value(f"textured res {res}: normals", torch.from_numpy(tex["normals"]), n64, n32.double())
    assert np.array_equal(tex["colors"], U.quantize_rgb(torch.from_numpy(tex["albedo"])).numpy())


def test_textured_geometry_end_to_end(R, tmp_path):
    ren = U.renderer(R, "sharp", device())
    res = 70
    dense = ren.extract_textured_geometry(LO, HI, res)
    _check_textured(R, ren, dense, res, sparse=False)
    sparse = ren.extract_textured_geometry(LO, HI, res, sparse=True, brick=8)
    _check_textured(R, ren, sparse, res, sparse=True)
    for k in dense:
        assert np.array_equal(dense[k], sparse[k]), f"{k}: the sparse grid's mesh differs from the dense grid's"
    # device tensors on request: the same arrays
    on_dev = ren.extract_textured_geometry(LO, HI, res, to_host=False)
    assert all(x.is_cuda for x in on_dev.values())
    for k in dense:
        assert np.array_equal(on_dev[k].cpu().numpy(), dense[k]), k
    # the PLY round trip
    path = tmp_path / "mesh.ply"
    R.write_ply(path, dense["vertices"], dense["triangles"], normals=dense["normals"], colors=dense["colors"])
    m = R.read_ply(path)
    assert np.array_equal(m["vertices"], dense["vertices"].astype(np.float32))
    assert np.array_equal(m["triangles"], dense["triangles"]) and np.array_equal(m["normals"], dense["normals"])
    assert np.array_equal(m["colors"], dense["colors"])


def test_refinement_moves_the_vertices_onto_the_level_set(R):
    """Marching cubes leaves its vertices O(h^2) off the level set (linear interpolation along grid edges); two Newton
    steps take them to the fp32 evaluation floor.  The ratio is printed, not asserted: only the strict decrease is."""
    ren = U.renderer(R, "sharp", device())
    mc, _, p64 = U.model("sharp")
    res = 70
    step = float(((HI - LO).double() / (res - 1)).pow(2).sum().sqrt())
    rms = {}
    for refine in (0, 2):
        tex = ren.extract_textured_geometry(LO, HI, res, refine=refine)
        v = torch.from_numpy(tex["vertices"])
        if refine == 0:
            v0 = v
        else:
            assert v.shape == v0.shape
            moved = (v - torch.tensor(v0.numpy()).type(torch.float32).double()).norm(dim=1)
            print(f"refine=2: largest move {float(moved.max()):.3e} (max_step {step:.3e})")
            assert float(moved.max()) <= step
            assert np.array_equal(tex["vertices"], tex["vertices"].astype(np.float32).astype(np.float64)), \
                "refined vertices are the float64 of fp32 points"
        with torch.no_grad():
            f = O.sdf_only(p64, mc.sdf, v.double())[:, 0]
        rms[refine] = float(f.pow(2).mean().sqrt())
    print(f"rms |sdf| over {v.shape[0]} vertices at res {res}: refine=0 {rms[0]:.3e}, refine=2 {rms[2]:.3e} "
          f"(ratio {rms[0] / max(rms[2], 1e-300):.1f})")
    assert rms[2] < rms[0]


def test_bf16_route_against_the_fp32_oracle(R):
    ren = U.renderer(R, "sharp_bf16", device())
    pts = U.point_batch("sharp_bf16", 200)
    out = ren.vertex_attributes(pts.to(device()), chunk=128)
    assert torch.equal(out["points"].cpu(), pts)
    ref = U.oracle_attributes("sharp", pts, tag=200)
    errs = {k: float((out[k].cpu() - ref[k][1]).abs().max()) for k in KEYS}
    print("bf16 route vs the fp32 oracle: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["sdf"] <= SDF_ATOL and errs["gradient"] <= NRM_ATOL and errs["albedo"] <= OUT_ATOL
    _check_epilogue(out)
    again = ren.vertex_attributes(pts.to(device()), chunk=128)
    for k in out:
        assert torch.equal(out[k], again[k]), k


def test_renderer_without_the_albedo_network(R):
    mc, p, _ = U.model("tiny")
    sdf, dev, col, full = R.build_from_named_params(mc, p, device())
    geo = R.NeuSRenderer(None, sdf, dev, None, n_samples=16, n_importance=16, n_outside=0, up_sample_steps=4, perturb=0.0)
    pts = U.point_batch("tiny", 65)
    out = geo.vertex_attributes(pts.to(device()), chunk=64)
    assert set(out) == {"points", "sdf", "gradient", "normal"}
    _check_parity("no albedo network", out, U.oracle_attributes("tiny", pts, tag=65), keys=("sdf", "gradient"))
    _check_epilogue(out)
    with pytest.raises(ValueError, match="albedo"):
        geo.vertex_attributes(pts.to(device()), albedo=True)
    # albedo=False on a full renderer: the same geometry outputs, no albedo sweep
    plain = full.vertex_attributes(pts.to(device()), albedo=False, chunk=64)
    assert set(plain) == set(out)
    for k in out:
        assert torch.equal(plain[k], out[k]), k
    # nothing is launched for an empty vertex array
    empty = full.vertex_attributes(torch.zeros(0, 3, device=device()))
    assert empty["points"].shape == (0, 3) and empty["rgb"].shape == (0, 3) and empty["sdf"].shape == (0, 1)


def test_runs_under_grad_mode_without_touching_autograd(R):
    ren = U.renderer(R, "tiny", device())
    pts = U.point_batch("tiny", 64).to(device()).requires_grad_(True)
    with torch.enable_grad():
        out = ren.vertex_attributes(pts, chunk=64)
    assert all(not v.requires_grad and v.grad_fn is None for v in out.values())
    assert all(q.grad is None for q in ren.sdf_network.parameters())
