"""The hole filling on the device (rnb_neus_fork_amd.mesh_fill, csrc/mesh_fill.hip) against the numpy reference of
tests/mesh_fill_ref.py, which tests/test_mesh_fill_host.py checks against facts.  For every case: loop offsets, ordered loop
vertices, statuses, edge counts, the new triangles, `filled` and `info` with array_equal; the old vertices, triangles and
attributes bit-equal to the inputs; two runs bit-equal in everything; centroids per coordinate within n 2^-52 mean|x| of the
reference's fsum / n (a sum in any order errs by at most (n - 1) 2^-53 sum|x|, the division adds one rounding, the factor 2 is
for second-order terms), attribute means within the same plus one fp32 rounding, 2^-24 |ref|.  Then the project's own
mesh_topology on the filled mesh: the summed Euler characteristic rose by n_filled, no flipped or non-manifold edge came, and
where every loop was filled the mesh is watertight, its volume within the audit's bound of the reference's volume of the
reference's filled mesh.  (The audit facts are for inputs without invalid triangles: an invalid triangle copied as it is may
come to name a new vertex, tests/test_mesh_fill_host.py.)  The shapes are the smallest at which each part can go wrong;
every case prints one FILL line with the largest centroid error as a fraction of its bound."""
import os
import time

import numpy as np
import pytest
import torch

from tests import mesh_cull_ref as CU
from tests import mesh_fill_ref as F
from tests import mesh_large_shapes as LS
from tests import mesh_topology_ref as M
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device
from tests.mesh_attrs_util import HI, LO

pytestmark = pytest.mark.gpu

_REF = {}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _np(x):
    return x.detach().cpu().numpy()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device())


def _ref(tag, v, t, max_edges, attributes):
    if tag not in _REF:
        _REF[tag] = F.fill(v, t, max_edges=max_edges, attributes=attributes)
    return _REF[tag]


def _euler(report):
    return int(report["components"]["euler"].sum())


def _ratio(got, ref, bound):
    """the largest |got - ref| / bound (0 where both vanish); NaN in the same places"""
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    err = np.abs(got - ref)
    ok = ~np.isnan(ref)
    assert (err[ok & (bound == 0)] == 0).all()
    use = ok & (bound > 0)
    return float((err[use] / bound[use]).max()) if use.any() else 0.0


def _check(R, tag, v, t, max_edges=None, attributes=None):
    """boundary_loops and fill_holes (twice) against the reference; returns (device result, reference, report after)"""
    t0 = time.perf_counter()
    ref = _ref(tag, v, t, max_edges, attributes)
    lp, V, T = ref["loops"], len(v), len(t)
    vv, tt = _dev(np.asarray(v, dtype=np.float64)), _dev(np.asarray(t, dtype=np.int32))
    loops = R.boundary_loops(tt, vertices=vv)
    assert loops["n_loops"] == lp["n_loops"]
    for k in ("loop_offsets", "loop_vertices", "loop_status", "loop_edges"):
        got = _np(loops[k])
        assert got.dtype == lp[k].dtype and np.array_equal(got, lp[k]), f"{tag}: {k} differs from the reference"
    bound = np.array([F.mean_bound(v, m) for m in lp["_members"]]).reshape(-1, 3)
    worst = _ratio(_np(loops["loop_centroid"]), lp["loop_centroid"], bound)
    again = R.boundary_loops(tt, V)
    assert "loop_centroid" not in again and all(torch.equal(again[k], loops[k]) for k in again if k != "n_loops")
    at = None if attributes is None else {"a": _dev(attributes)}
    out = R.fill_holes(vv, tt, max_edges=max_edges, attributes=at)
    twice = R.fill_holes(vv, tt, max_edges=max_edges, attributes=at)
    assert out["info"] == ref["info"] == twice["info"], (tag, out["info"], ref["info"])
    assert all(type(x) is int for x in out["info"].values())
    got_v, got_t, n_f = _np(out["vertices"]), _np(out["triangles"]), ref["info"]["n_filled"]
    assert got_v.dtype == np.float64 and got_t.dtype == np.int32 and out["filled"].dtype == torch.int32
    assert np.array_equal(got_t, ref["triangles"]) and np.array_equal(_np(out["filled"]), ref["filled"])
    assert got_v[:V].tobytes() == np.asarray(v, dtype=np.float64).tobytes(), f"{tag}: the old vertices are not bit-equal"
    assert got_v.shape == (V + n_f, 3) and got_v[V:].tobytes() == _np(loops["loop_centroid"])[ref["filled"]].tobytes()
    for k in ("vertices", "triangles", "filled"):
        assert _np(out[k]).tobytes() == _np(twice[k]).tobytes(), f"{tag}: {k} differs between two runs"
    worst_a = 0.0
    if attributes is not None:
        a = _np(out["attributes"]["a"])
        assert a.dtype == np.float32 and a.shape == (V + n_f, attributes.shape[1]) and a[:V].tobytes() == attributes.tobytes()
        assert a.tobytes() == _np(twice["attributes"]["a"]).tobytes()
        means = ref["attribute_means"]
        ab = np.array([F.mean_bound(attributes, lp["_members"][l]) for l in ref["filled"]]).reshape(means.shape)
        worst_a = _ratio(a[V:].astype(np.float64), means, ab + 2.0 ** -24 * np.abs(means))
        assert worst_a <= 1.0, f"{tag}: attribute means {worst_a:.2f} of their bound"
    else:
        assert out["attributes"] == {}
    before = R.mesh_topology(tt, vertices=vv)
    after = R.mesh_topology(out["triangles"], vertices=out["vertices"])
    closed = bool(R.watertight(after))
    vol = ""
    if before["n_invalid"] == 0:
        assert _euler(after) - _euler(before) == n_f, f"{tag}: the Euler characteristic did not rise by n_filled"
        assert after["n_flipped"] == before["n_flipped"] and after["n_nonmanifold"] == before["n_nonmanifold"]
        assert after["n_boundary_components"] == before["n_boundary_components"] - n_f
        if n_f == lp["n_loops"] and before["n_flipped"] == 0 and before["n_nonmanifold"] == 0 and before["n_degenerate"] == 0:
            assert closed, f"{tag}: every loop was filled and the mesh is not watertight"
            audit = M.topology(ref["triangles"], len(ref["vertices"]), ref["vertices"])
            got_vol = _np(after["components"]["volume"])
            r = _ratio(got_vol, audit["volume"], audit["volume_bound"])
            vol = f"; volumes {got_vol[:2].tolist()}, {r:.2e} of the audit's bound"
            assert r <= 1.0, f"{tag}: volume error {r:.2f} of its bound"
    print(f"FILL {tag}: V {V} T {T} info {out['info']}; centroid error at most {worst:.3f} of its bound, attribute means "
          f"{worst_a:.3f}{vol}; watertight {closed}; {time.perf_counter() - t0:.2f} s")
    assert worst <= 1.0, f"{tag}: centroids {worst:.2f} of their bound"
    return out, ref, after


def test_the_minimal_loop(R):
    out, ref, after = _check(R, "open tetrahedron", *F.open_tetrahedron())
    assert out["info"] == dict(zip(F.INFO_KEYS, (1, 1, 0, 0, 0, 3, 3))) and _np(out["triangles"])[-3:, 2].tolist() == [4, 4, 4]
    assert abs(float(after["components"]["volume"][0]) - 1 / 6) <= 2 ** -52


@pytest.mark.parametrize("n", [3, 63, 64, 65, 255, 256, 257, 1025])
def test_wave_and_workgroup_edges_of_the_ranking(R, n):
    out, _, after = _check(R, f"tube {n}", *F.tube(n, 2))
    assert out["info"] == dict(zip(F.INFO_KEYS, (2, 2, 0, 0, 0, 2 * n, n)))
    assert abs(float(after["components"]["volume"][0]) - F.ngon_area(n)) <= 1e-12 * n


def test_eighteen_rounds_of_pointer_jumping(R):
    """2^17 + 3 edges per loop: ceil(log2) = 18 rounds, an even count after the odd 17 a ring of 2^17 would take; tube 65
    (7 rounds) and 1025 (11) are the odd ones: both parities of the two buffers are read"""
    n = 2 ** 17 + 3
    out, ref, _ = _check(R, "ring 2^17 + 3", *F.tube(n, 2))
    assert out["info"]["longest_filled"] == n and out["info"]["n_new_triangles"] == 2 * n
    lv = ref["loops"]["loop_vertices"]
    assert lv[:n].tolist() == list(range(n)) and lv[n:n + 3].tolist() == [n, 2 * n - 1, 2 * n - 2], "one loop with, one against the index order"


@pytest.mark.parametrize("n", [65, 1025])
def test_walk_order_that_is_not_index_order(R, n):
    mesh = M.interleave([F.tube(n, 2)], seed=n)
    out, ref, after = _check(R, f"tube {n} interleaved", *mesh)
    lv = ref["loops"]["loop_vertices"]
    assert (np.diff(lv[:n]) < 0).any() and (np.diff(lv[:n]) > 0).any(), "the walk jumps about in the index order"
    outward = float(after["components"]["volume"][0])
    assert abs(outward - F.ngon_area(n)) <= 1e-12 * n
    _, _, inner = _check(R, f"tube {n} interleaved, inside out", *F.inside_out(mesh))
    assert abs(float(inner["components"]["volume"][0]) + outward) <= 1e-12 * n, "the caps keep the sign of the surface"


def test_many_short_loops_on_the_punched_sheet(R):
    m, k, q = 40, 47, 5
    out, _, after = _check(R, "punched sheet", *F.punched_sheet(m, k, q), max_edges=4)
    holes = F.punched_holes(m, k, q)
    assert holes > 300 and out["info"]["n_filled"] == holes and out["info"]["n_too_long"] == 1
    assert out["info"]["n_loops"] == holes + 1 and out["info"]["longest_filled"] == 4
    assert after["n_boundary_components"] == 1 and not R.watertight(after), "the long outer rim is left"


def test_a_million_three_loops_across_four_scan_chunks(R):
    """the 2^20 + 4,101 isolated triangles: that many 3-loops, their boundary vertices in four chunks of the block-sum scan,
    the loops in two; the expectation is analytic (the reference's Python walk would take minutes)"""
    big = LS.big("ISOLATED")
    v, t = big["vertices"], big["triangles"]
    V, T = len(v), len(t)
    t0 = time.perf_counter()
    vv, tt = _dev(v), _dev(t)
    out = R.fill_holes(vv, tt)
    assert out["info"] == dict(zip(F.INFO_KEYS, (T, T, 0, 0, 0, 3 * T, 3)))
    first = t.argmin(axis=1)                                     # every loop starts at its smallest vertex and follows its triangle
    w = np.stack([np.take_along_axis(t, ((first + j) % 3)[:, None], axis=1)[:, 0] for j in range(3)], axis=1)
    order = np.argsort(w[:, 0], kind="stable")                   # loops are numbered by smallest vertex
    w = w[order]
    apex = (V + np.arange(T)).astype(np.int32)
    want = np.stack([np.stack([w[:, (j + 1) % 3], w[:, j], apex], axis=1) for j in range(3)], axis=1).reshape(-1, 3)
    got_t, got_v = _np(out["triangles"]), _np(out["vertices"])
    assert np.array_equal(got_t[:T], t) and np.array_equal(got_t[T:], want) and got_v[:V].tobytes() == v.tobytes()
    assert np.array_equal(_np(out["filled"]), np.arange(T, dtype=np.int32))
    corners = v[w].astype(np.longdouble)
    err = np.abs(got_v[V:] - (corners.sum(axis=1) / 3).astype(np.float64))
    bound = 3 * 2.0 ** -52 * np.abs(v[w]).mean(axis=1) + 2.0 ** -63 * np.abs(got_v[V:])      # (+ the extended reference's own rounding)
    assert (err <= bound).all()
    after = R.mesh_topology(out["triangles"], vertices=out["vertices"])
    c = after["components"]
    assert R.watertight(after) and c["n_components"] == T and bool((c["euler"] == 2).all()) and after["n_manifold"] == 6 * T
    assert bool((c["volume"] == 0).all()) or float(c["volume"].abs().max()) < 1e-6, "every result is a closed two-sided triangle"
    print(f"FILL isolated: V {V} T {T} info {out['info']}; centroid error at most {float((err / bound).max()):.3f} of its "
          f"bound; {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("name", ["bow tie", "moebius", "all interleaved"])
def test_loops_that_are_skipped(R, name):
    out, ref, _ = _check(R, name, *M.small_shapes()[name])
    want = {"bow tie": (1, 0, 1, 0), "moebius": (1, 0, 0, 1), "all interleaved": (3, 1, 1, 1)}[name]
    assert tuple(out["info"][k] for k in F.INFO_KEYS[:4]) == want
    if name != "all interleaved":
        assert out["vertices"].shape[0] == len(M.small_shapes()[name][0]) and out["filled"].numel() == 0


def test_torus_with_holes_status_by_status(R):
    mesh = M.torus_with_holes(60, 30, 100)
    ref = _ref("torus holes", *mesh, None, None)
    assert (ref["info"]["n_loops"], ref["info"]["n_filled"]) == (86, 76), "the reference itself fills 76 of 86"
    out, _, after = _check(R, "torus holes", *mesh)
    assert out["info"]["n_tangled"] == 10 and after["n_boundary"] == 64
    limited, _, _ = _check(R, "torus holes, at most 3 edges", *mesh, max_edges=3)
    assert 0 < limited["info"]["n_filled"] < 76 and limited["info"]["n_too_long"] == 76 - limited["info"]["n_filled"]


def test_degenerate_input_passes_through(R):
    v, t = M.degenerate_input()
    out, ref, _ = _check(R, "degenerate input", v, t)
    assert _np(out["triangles"])[:len(t)].tobytes() == t.tobytes() and out["info"]["n_filled"] == 1
    assert _np(out["vertices"])[10:12].tobytes() == v[10:12].tobytes(), "the unreferenced vertices stay in place"


def test_empty_inputs(R):
    none = np.zeros((0, 3), dtype=np.int32)
    for tag, v, t in (("T = 0", np.zeros((5, 3)), none), ("V = 0", np.zeros((0, 3)), np.array([[0, 1, 2], [0, 0, 0]], dtype=np.int32)),
                      ("V = 0, T = 0", np.zeros((0, 3)), none), ("icosphere", *M.icosphere(2))):
        out, _, _ = _check(R, tag, v, t)
        assert out["info"] == dict(zip(F.INFO_KEYS, (0,) * 7)) and out["filled"].shape == (0,)
        assert np.array_equal(_np(out["vertices"]), v) and np.array_equal(_np(out["triangles"]), t)
        loops = R.boundary_loops(_dev(t), vertices=_dev(v))
        assert loops["n_loops"] == 0 and _np(loops["loop_offsets"]).tolist() == [0] and loops["loop_vertices"].shape == (0,)
        assert loops["loop_centroid"].shape == (0, 3)


@pytest.mark.parametrize("shape", ["tube", "torus"])
def test_attributes(R, shape):
    v, t = F.tube(257, 2) if shape == "tube" else M.torus_with_holes(60, 30, 100)
    a = np.random.default_rng(5).normal(size=(len(v), 5)).astype(np.float32) * np.float32(3.0)
    out, ref, _ = _check(R, f"attributes on the {shape}", v, t, attributes=a)
    assert out["attributes"]["a"].shape[0] == len(v) + ref["info"]["n_filled"] and ref["info"]["n_filled"] > 1
    # a trailing shape survives, and a 1-d attribute
    vv, tt = _dev(v), _dev(t)
    more = R.fill_holes(vv, tt, attributes={"b": _dev(a[:, :4].reshape(-1, 2, 2)), "c": _dev(a[:, 0])})
    assert more["attributes"]["b"].shape == (len(v) + ref["info"]["n_filled"], 2, 2)
    assert torch.equal(more["attributes"]["b"].reshape(-1, 4), out["attributes"]["a"][:, :4])
    assert torch.equal(more["attributes"]["c"], out["attributes"]["a"][:, 0])


# ---- through the renderer ---------------------------------------------------------------------------------------------------
RES = 40


def _tiny_renderer(R):
    """the tiny checkpoint's renderer (tests/golden/ref_ckpt_tiny.pth), as tests/test_gpu_mesh_pipeline.py builds it"""
    from rnb_neus_fork_amd import checkpoint as CK
    dev = device()
    nc = np.load(os.path.join(GOLDEN, "ref_ckpt_tiny_step3.npz"), allow_pickle=False)["nerf.conf"]
    torch.manual_seed(99)
    nerf = R.NeRF(D=int(nc[0]), W=int(nc[1]), d_in=int(nc[2]), d_in_view=int(nc[3]), multires=int(nc[4]),
                  multires_view=int(nc[5]), output_ch=int(nc[6]), skips=[int(nc[7])], use_viewdirs=True).to(dev)
    sdf = R.SDFNetwork(d_in=3, d_out=65, d_hidden=64, n_layers=8, skip_in=[4], multires=6).to(dev)
    devn = R.SingleVarianceNetwork(0.1).to(dev)
    col = R.RenderingNetwork(d_feature=64, mode="no_view_dir", d_in=6, d_out=3, d_hidden=64, n_layers=2, multires_view=4).to(dev)
    ren = R.NeuSRenderer(nerf, sdf, devn, col, n_samples=16, n_importance=16, n_outside=0, up_sample_steps=4, perturb=1.0)
    params = list(nerf.parameters()) + list(sdf.parameters()) + list(devn.parameters()) + list(col.parameters())
    CK.load_checkpoint(os.path.join(GOLDEN, "ref_ckpt_tiny.pth"), nerf, sdf, devn, col, R.FlatAdam(params, lr=1.0), map_location=dev)
    return ren


def test_the_fill_keyword_of_the_extract_calls(R):
    from rnb_neus_fork_amd import mesh_pipeline as P
    ren = _tiny_renderer(R)
    assert ren.last_mesh_fill is None
    plain_v, plain_t = ren.extract_geometry(LO, HI, RES, threshold=0.0, backend="native")
    same_v, same_t = ren.extract_geometry(LO, HI, RES, threshold=0.0, backend="native", fill=None)
    assert same_v.tobytes() == plain_v.tobytes() and same_t.tobytes() == plain_t.tobytes() and ren.last_mesh_fill is None
    # the three-camera cull of tests/test_gpu_mesh_pipeline.py (left half of every mask cut away) opens the mesh
    s = CU.scene()
    masks = s["masks"][:3].copy()
    masks[:, :, :24] = 0
    cull = dict(projections=_dev(s["projections"][:3]), eyes=_dev(s["eyes"][:3]), masks=_dev(masks * np.uint8(255)), max_outside=1)
    v, t = P.device_mesh(ren, LO, HI, RES, 0.0, False, None, 1.0, {"cull": cull})
    by_hand = R.fill_holes(v, t)
    assert by_hand["info"]["n_loops"] > 0 and by_hand["info"]["n_filled"] > 0, "the cull opens the mesh"
    want_v = P.rescale_to_bounds_host(_np(by_hand["vertices"]), LO, HI, RES)
    got_v, got_t = ren.extract_geometry(LO, HI, RES, threshold=0.0, backend="native", cull=cull, fill={})
    assert got_v.tobytes() == want_v.tobytes() and np.array_equal(got_t, _np(by_hand["triangles"]))
    assert ren.last_mesh_fill == by_hand["info"] and len(got_t) == t.shape[0] + by_hand["info"]["n_new_triangles"]
    limited = ren.extract_geometry(LO, HI, RES, threshold=0.0, backend="native", cull=cull, fill={"max_edges": 3})
    assert ren.last_mesh_fill["longest_filled"] <= 3 and len(limited[1]) <= len(got_t)
    # the textured call: the cap centroids are vertices like any other, with normals and colours
    tex = ren.extract_textured_geometry(LO, HI, RES, threshold=0.0, cull=cull, fill={})
    assert np.array_equal(tex["triangles"], got_t) and tex["vertices"].tobytes() == got_v.tobytes()
    assert tex["normals"].shape == (len(got_v), 3) and np.isfinite(tex["normals"]).all()
    no_fill = ren.extract_textured_geometry(LO, HI, RES, threshold=0.0, cull=cull)
    assert np.array_equal(no_fill["triangles"], _np(t)) and no_fill["vertices"].shape[0] == v.shape[0]
    print(f"FILL renderer: {t.shape[0]} triangles after the cull, info {by_hand['info']}")
