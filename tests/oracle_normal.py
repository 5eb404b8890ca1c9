"""The oracle's normal with its graph kept to the points.  Torch on the CPU only; not a test module.

oracle/rnb_oracle.py::sdf_gradient detaches its input: enough for parameter gradients.  The reference's gradient()
(models/fields.py:114-127) keeps the graph to the points when they require grad, so the normal's Hessian-vector term is
part of the reference's gradient with respect to rays and depths.  Every comparison of an input gradient runs the oracle
with `sdf_gradient_with_graph` in place of O.sdf_gradient: as the `graph_normal` fixture (a test asks for it by name, after
`from tests.oracle_normal import graph_normal`), or inside `with graph_normal_installed():` where a plain module builds a
cached oracle graph (tests/input_adjoint_matrix.py)."""
import contextlib

import pytest
import torch

from oracle import rnb_oracle as O


def sdf_gradient_with_graph(p, conf, pts, create_graph=True):
    x = pts if pts.requires_grad else pts.detach().requires_grad_(True)
    with torch.enable_grad():
        y = O.sdf_only(p, conf, x)
        (g,) = torch.autograd.grad(y, x, torch.ones_like(y), create_graph=True, retain_graph=True)
    return g


@pytest.fixture
def graph_normal(monkeypatch):
    monkeypatch.setattr(O, "sdf_gradient", sdf_gradient_with_graph)


@contextlib.contextmanager
def graph_normal_installed():
    saved = O.sdf_gradient
    O.sdf_gradient = sdf_gradient_with_graph
    try:
        yield
    finally:
        O.sdf_gradient = saved
