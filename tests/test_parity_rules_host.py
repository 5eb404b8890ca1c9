"""tests/parity.py itself, on hand-made float64 tensors (no GPU): the constants, the two rules just inside and just outside
their bounds — the expected bound is written out here independently, as the specification — and two source scans that keep
the rule in one place and test modules from importing test modules."""
import glob
import os
import re

import pytest
import torch

from tests import golden_util, parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants():
    assert (parity.K_OUT, parity.FLOOR_OUT, parity.K_GRAD, parity.GRAD_CAP) == (3.0, 2e-6, 3.0, 1e-2)
    assert golden_util.GRAD_CAP is parity.GRAD_CAP


def _case(scale, e_ref):
    """r64 with max|r64| = scale (attained at element 0, error-free there), r32 exactly e_ref away from it at element 1"""
    r64 = torch.tensor([[scale, -0.25 * scale, 0.125 * scale], [0.0, 0.5 * scale, -0.75 * scale]], dtype=torch.float64)
    r32 = r64.clone()
    r32[0, 1] += e_ref
    assert float((r32 - r64).abs().max()) == e_ref
    return r64, r32


def _got(r64, err):
    got = r64.clone()
    got[1, 2] -= err
    return got


# (max|r64|, e_ref, keywords, the bound by the rule as the documents state it)
VALUE_CASES = [
    (0.5, 2.0 ** -20, {}, 3.0 * 2.0 ** -20 + 2e-6 * 1.0),                             # max|r64| < 1: the floor is absolute
    (64.0, 2.0 ** -12, {}, 3.0 * 2.0 ** -12 + 2e-6 * 64.0),                           # max|r64| > 1: the floor is relative
    (64.0, 2.0 ** -12, dict(k=10.0), 10.0 * 2.0 ** -12 + 2e-6 * 64.0),
    (64.0, 2.0 ** -12, dict(floor_scale=0.25), 3.0 * 2.0 ** -12 + 2e-6 * 0.25),
    (0.5, 0.0, {}, 2e-6),                                                             # an exact fp32 reference: the floor alone
]


@pytest.mark.parametrize("scale,e_ref,kw,bound", VALUE_CASES, ids=["below_1", "above_1", "k", "floor_scale", "exact_ref"])
def test_check_value_at_its_bound(scale, e_ref, kw, bound):
    r64, r32 = _case(scale, e_ref)
    assert parity.value_bound(r64, e_ref, **kw) == pytest.approx(bound, rel=1e-14)
    inside = _got(r64, bound * (1.0 - 1e-9))     # (the subtraction rounds to an ulp of r64: 1e-11 of the bound at most)
    assert parity.check_value("inside", inside, r64, r32, **kw) == pytest.approx(1.0 - 1e-9, abs=2e-10)
    with pytest.raises(AssertionError, match="outside.*bound"):
        parity.check_value("outside", _got(r64, bound * (1.0 + 1e-6)), r64, r32, **kw)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_check_value_refuses_non_finite_values(bad):
    r64, r32 = _case(64.0, 2.0 ** -12)
    got = r64.clone()
    got[0, 2] = bad
    with pytest.raises(AssertionError, match="not finite"):
        parity.check_value("x", got, r64, r32)


def test_check_value_refuses_another_shape():
    r64, r32 = _case(64.0, 2.0 ** -12)
    for got in (r64.reshape(3, 2), r64[:1], r64.reshape(-1)):      # the second would broadcast against r64
        with pytest.raises(AssertionError, match="shape"):
            parity.check_value("x", got, r64, r32)
    assert parity.check_value("x", r64.reshape(-1).reshape(2, 3), r64, r32) == 0.0


def test_check_value_message_names_what_and_the_three_figures():
    r64, r32 = _case(0.5, 2.0 ** -20)
    with pytest.raises(AssertionError) as e:
        parity.check_value("tag: color", _got(r64, 1e-3), r64, r32)
    msg = str(e.value)
    assert "tag: color" in msg and "1.000e-03" in msg and f"{3.0 * 2.0 ** -20 + 2e-6:.3e}" in msg and f"{2.0 ** -20:.3e}" in msg


def test_rel_l2():
    a, b = torch.tensor([3.0, 4.0], dtype=torch.float64), torch.tensor([0.0, 4.0], dtype=torch.float64)
    assert parity.rel_l2(a, b) == 0.75
    assert parity.rel_l2(a.float(), b) == 0.75
    assert parity.rel_l2(b, torch.zeros(2)) == 4.0 / 1e-300      # the clamp, not a division by zero


@pytest.mark.parametrize("rel32,bound", [(0.0, 1e-4), (1e-5, 1e-4), (1e-3, 3e-3), (1.0, 1e-2)])
def test_grad_bound(rel32, bound):
    assert parity.grad_bound(rel32) == bound


@pytest.mark.parametrize("rel32", [0.0, 1e-3, 1.0], ids=["floor", "calibrated", "cap"])
def test_check_grad_at_its_bound(rel32):
    g64 = torch.tensor([3.0, 0.0, -4.0], dtype=torch.float64)      # |g64| = 5
    bound = min(1e-2, max(1e-4, 3.0 * rel32))

    def got(rel):
        g = g64.clone()
        g[1] = 5.0 * rel
        return g

    assert parity.check_grad("inside", got(bound * (1.0 - 1e-9)), g64, rel32) == pytest.approx(1.0 - 1e-9, abs=2e-10)
    with pytest.raises(AssertionError, match="outside.*bound"):
        parity.check_grad("outside", got(bound * (1.0 + 1e-6)), g64, rel32)
    with pytest.raises(AssertionError, match="shape"):
        parity.check_grad("x", g64[:1], g64, rel32)
    with pytest.raises(AssertionError):
        parity.check_grad("x", torch.full_like(g64, float("nan")), g64, rel32)


# ------------------------------------------------------------------------------------------------------- source scans
def _sources():
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")))
    assert len(paths) > 40
    return [(os.path.relpath(p, ROOT), open(p).read()) for p in paths]


def test_no_module_imports_a_test_module():
    """a test module imported as `tests.test_x` is a second copy of the module pytest collected as `test_x`"""
    pat = re.compile(r"^\s*(from|import)\s+tests\.test_", re.M)
    bad = [name for name, text in _sources() if pat.search(text)]
    assert not bad, f"these import a test module: {bad}; shared code belongs in a non-test module"


def test_the_output_rule_is_written_once():
    needle = "K_OUT" + " *"       # (put together here so that this file does not hold it)
    holders = [name for name, text in _sources() if needle in text]
    assert holders == [os.path.join("tests", "parity.py")], f"the output rule's formula is restated in {holders}"
