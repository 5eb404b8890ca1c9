"""The mesh topology entry points between guard bands (tests/guard_bands.py), by the rule of tests/test_gpu_guard_cull.py: the
call runs once on ordinary allocations and once under guarded() with its inputs passed through guard(); both bands of every
allocation must still hold their pattern, the registry must have seen the buffers the call is known to make — the workspace
of exactly the queried size among them — and every result must equal the unguarded run bit for bit (integer atomics only;
the volume is an integer sum).  Under guarded() the body of every torch.empty holds the pattern, so the flags, labels,
degrees, the table and the edge arrays are at the same time checked for words the kernels never wrote.  The mesh is the
degenerate-input mesh of tests/mesh_topology_ref.py: an index V and an index -1 among its triangles.  One positive control:
an output handed out short trips the bands.  Every case prints one line starting with GUARD."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from tests import guard_bands as GB
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
    """the three entry points: count, emit and components, then the count without boundary components"""
    return (R.mesh_topology(x["t"], vertices=x["v"], edges=True),
            R.mesh_topology(x["t"], x["v"].shape[0], edges=True, boundary=False, components=False))


def test_the_three_entry_points_on_the_degenerate_input(R):
    v, t = M.degenerate_input()
    V, T = len(v), len(t)
    ref = M.topology(t, V, v)
    ws = C.c_int64()
    R.native.check(R.native.load().rnb_mesh_topology_workspace_bytes(V, T, C.byref(ws)))
    t0 = time.perf_counter()
    clean = _call(R, {"v": _dev(v), "t": _dev(t)})
    torch.cuda.synchronize()
    with GB.guarded() as s:
        got = _call(R, {"v": _dev(v, GB.guard), "t": _dev(t, GB.guard)})
        torch.cuda.synchronize()
        GB.assert_intact("mesh_topology")
    GB.assert_same("mesh_topology", clean, got)
    print(f"GUARD topology degenerate input: {len(s.registry)} guarded allocations, {time.perf_counter() - t0:.2f} s")
    made = lambda **kw: [e for e in s.seen(**kw) if e.how != "guard"]     # noqa: E731
    E, n_comp = int(ref["counts"][0]), ref["n_components"]
    assert len(made(nbytes=ws.value, dtype=u8)) == 2, "the workspace is exactly the queried size, in both calls"
    assert len(made(shape=(T,), dtype=u8)) == 2 and len(made(shape=(V,), dtype=u8)) == 2
    assert len(made(shape=(V,), dtype=torch.int32)) == 3, "boundary labels, degrees, component labels"
    assert len(made(shape=(E, 2), dtype=torch.int32)) == 4 and len(made(shape=(E,), dtype=torch.int32)) == 2
    assert made(shape=(n_comp, 8), dtype=torch.int64) and made(shape=(n_comp,), dtype=torch.float64)
    full, plain = got
    assert full["n_invalid"] == 2 and plain["n_invalid"] == 2
    assert np.array_equal(full["edges"].cpu().numpy(), ref["edges"]) and torch.equal(full["edges"], plain["edges"])
    assert np.array_equal(full["triangle_flags"].cpu().numpy(), ref["triangle_flags"])
    assert np.array_equal(full["boundary_labels"].cpu().numpy(), ref["boundary_labels"])


@pytest.mark.parametrize("what", ["triangle_flags", "edges", "table"])
def test_an_output_handed_out_short_trips_the_bands(R, what):
    """the positive control: the same call with one output counted short — the kernel's last store lands in the band"""
    v, t = M.degenerate_input()
    ref = M.topology(t, len(v), v)
    shape, short = {"triangle_flags": ((len(t),), 1), "edges": ((int(ref["counts"][0]), 2), 4),
                    "table": ((ref["n_components"], 8), 8)}[what]
    with GB.guarded(shortchange=(shape, short)) as s:
        R.mesh_topology(_dev(t, GB.guard), vertices=_dev(v, GB.guard), edges=True)
        torch.cuda.synchronize()
        bad = s.damaged()
    assert len(bad) == 1 and bad[0]["band"] == "trailing" and tuple(bad[0]["shape"]) == shape, bad
    assert bad[0]["first"] >= bad[0]["nbytes"] and bad[0]["last"] < bad[0]["nbytes"] + short, bad
    print(f"GUARD topology positive control {what}: bytes {bad[0]['first']} .. {bad[0]['last']} of {list(shape)} reported")
