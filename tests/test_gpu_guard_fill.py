"""The hole-filling entry points between guard bands (tests/guard_bands.py), by the rule of tests/test_gpu_guard_topology.py:
the calls run once on ordinary allocations and once under guarded() with their inputs passed through guard(); both bands of
every allocation must still hold their pattern, the registry must have seen the buffers the calls are known to make — the two
workspaces of exactly the queried sizes among them — and every result must equal the unguarded run bit for bit (integer
atomics only; the means are integer sums).  Under guarded() the body of every torch.empty holds the pattern, so the CSR
arrays, statuses, centroids and the filled mesh are at the same time checked for words the kernels never wrote.  The meshes:
the degenerate-input mesh of tests/mesh_topology_ref.py (an index V and an index -1 among its triangles, one loop that is
walked and one that is sorted) and tube(65, 2) (two loops across a wave edge).  Every case prints one line starting with
GUARD."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from tests import guard_bands as GB
from tests import mesh_fill_ref as F
from tests import mesh_topology_ref as M
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device

pytestmark = pytest.mark.gpu

u8 = torch.uint8


@pytest.fixture(autouse=True)
def _release():
    yield
    GB.release()


def _dev(x, g=lambda t: t):
    return g(torch.from_numpy(np.ascontiguousarray(x)).to(device()))


def _call(R, x):
    loops = R.boundary_loops(x["t"], vertices=x["v"])
    filled = R.fill_holes(x["v"], x["t"], attributes={"a": x["a"]})
    short = R.fill_holes(x["v"], x["t"], max_edges=3)
    return loops, {k: filled[k] for k in ("vertices", "triangles", "filled")}, filled["attributes"]["a"], short["triangles"]


@pytest.mark.parametrize("shape", ["degenerate input", "tube 65"])
def test_loops_and_fill_between_guard_bands(R, shape):
    v, t = M.degenerate_input() if shape == "degenerate input" else F.tube(65, 2)
    V, T = len(v), len(t)
    a = np.random.default_rng(1).normal(size=(V, 5)).astype(np.float32)
    ref = F.fill(v, t, attributes=a)
    lp, n_f, n_new = ref["loops"], ref["info"]["n_filled"], ref["info"]["n_new_triangles"]
    ws, tws = C.c_int64(), C.c_int64()
    R.native.check(R.native.load().rnb_mesh_fill_workspace_bytes(V, T, C.byref(ws)))
    R.native.check(R.native.load().rnb_mesh_topology_workspace_bytes(V, T, C.byref(tws)))
    t0 = time.perf_counter()
    clean = _call(R, {"v": _dev(v), "t": _dev(t), "a": _dev(a)})
    torch.cuda.synchronize()
    with GB.guarded() as s:
        got = _call(R, {"v": _dev(v, GB.guard), "t": _dev(t, GB.guard), "a": _dev(a, GB.guard)})
        torch.cuda.synchronize()
        GB.assert_intact("mesh_fill")
    GB.assert_same("mesh_fill", clean, got)
    print(f"GUARD fill {shape}: {len(s.registry)} guarded allocations, {time.perf_counter() - t0:.2f} s")
    made = lambda **kw: [e for e in s.seen(**kw) if e.how != "guard"]     # noqa: E731
    L, B = lp["n_loops"], len(lp["loop_vertices"])
    assert ws.value != tws.value
    assert len(made(nbytes=ws.value, dtype=u8)) == 3 and len(made(nbytes=tws.value, dtype=u8)) == 3, "the workspaces are exactly the queried sizes, in all three calls"
    assert len(made(shape=(L + 1,), dtype=torch.int64)) >= 2 and len(made(shape=(B,), dtype=torch.int32)) >= 2
    assert made(shape=(L, 3), dtype=torch.float64) and made(shape=(L, 5), dtype=torch.float32)
    assert made(shape=(V + n_f, 3), dtype=torch.float64) and made(shape=(T + n_new, 3), dtype=torch.int32)
    loops, filled, attr, short = got
    assert np.array_equal(loops["loop_vertices"].cpu().numpy(), lp["loop_vertices"])
    assert np.array_equal(loops["loop_status"].cpu().numpy(), lp["loop_status"])
    assert np.array_equal(filled["triangles"].cpu().numpy(), ref["triangles"])
    assert attr.shape == (V + n_f, 5) and short.shape[0] <= T + n_new
