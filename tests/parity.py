"""The parity rule of the GPU tests, stated once.  Torch on the CPU only; needs no GPU.

Tolerances.  Integer sample indices: bit-exact given identical inputs.  Floating point: SURVEY.md 8c states
|d| <= 1e-5 + 1e-4 |ref| for outputs and rel-L2 <= 1e-4 for parameter gradients — but the fixtures show that the
fp32 REFERENCE itself is further than that from the exact result wherever the quantity is ill-conditioned (cdf_fine
4.9e-5 at inv_s = 403; d loss / d lin8.weight_g 1.4e-3).  Every fixture therefore also holds the reference's own code
run in fp64 on the same samples (oracle/gen_golden.py::reference_fp64), and the tests bound the device's distance from
fp64 by the fp32 reference's distance from fp64:
    outputs:    max|dev - ref64| <= K_OUT x max|ref32 - ref64| + FLOOR_OUT x max(1, max|ref64|)
    gradients:  relL2(dev, ref64) <= min(GRAD_CAP, max(1e-4, K_GRAD x relL2(ref32, ref64)))          per tensor
i.e. "as accurate as the reference's fp32, up to a stated factor", instead of hand-set absolute bounds.  Where no fixture
exists, ref32 / ref64 are the CPU oracle (oracle/rnb_oracle.py) run in fp32 / fp64 on the device's own samples.

This module must not import tests/golden_util.py (which takes GRAD_CAP from here and is imported by tools)."""
import torch

K_OUT, FLOOR_OUT = 3.0, 2e-6     # outputs: factor over the fp32 reference's own max error + a few fp32 ulps
K_GRAD = 3.0                     # gradients: factor over the fp32 reference's own relative L2 error
GRAD_CAP = 1e-2                  # ... capped: a gradient the fp32 reference resolves to worse than GRAD_CAP / K_GRAD
                                 # is not a parity target (tests/golden_util.py refuses such a fixture at load time)


def _f64(t):
    return t.detach().cpu().double()


def max_err(a, r64):
    """max|a - r64| in float64 on the CPU"""
    return float((_f64(a) - _f64(r64)).abs().max())


def ref_term(e_ref, k=K_OUT):
    """the calibrated part of a bound: K_OUT * the fp32 reference's own error (the bounds that add another floor of
    their own — the Adam moments, the calibrated loss rule — take this part from here)"""
    return k * e_ref


def value_bound(r64, e_ref, k=K_OUT, floor_scale=None):
    """the output bound for a reference r64 whose fp32 run is e_ref (max-abs) away from it"""
    return ref_term(e_ref, k) + FLOOR_OUT * (max(1.0, float(r64.abs().max())) if floor_scale is None else floor_scale)


def value_errors(got, r64, r32, k=K_OUT, floor_scale=None):
    """(e_dev, e_ref, bound) of the output rule, for the callers that print them"""
    e_ref = max_err(r32, r64)
    return max_err(got, r64), e_ref, value_bound(r64, e_ref, k, floor_scale)


def check_value(what, got, r64, r32, k=K_OUT, floor_scale=None):
    """The output rule on one tensor (or scalar): same shape as r64, finite, max|got - r64| within value_bound.
    Returns e_dev / bound."""
    got = _f64(got)
    assert got.shape == r64.shape, f"{what}: shape {tuple(got.shape)} != {tuple(r64.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    e_dev, e_ref, bound = value_errors(got, r64, r32, k, floor_scale)
    assert e_dev <= bound, f"{what}: |dev - fp64| {e_dev:.3e} > bound {bound:.3e} (fp32 reference: {e_ref:.3e})"
    return e_dev / bound


def rel_l2(a, b):
    """|a - b| / |b| in float64 (where the tensors live)"""
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def grad_bound(rel32):
    """the gradient bound for a tensor whose fp32 reference is rel32 (rel-L2) away from its fp64 one"""
    return min(GRAD_CAP, max(1e-4, K_GRAD * rel32))


def check_grad(what, got, g64, rel32):
    """The gradient rule on one tensor whose fp64 reference g64 does not vanish (a vanishing one is the caller's to
    treat, in front of the call).  Returns rel / bound."""
    assert got.shape == g64.shape, f"{what}: shape {tuple(got.shape)} != {tuple(g64.shape)}"
    rel, bound = rel_l2(got, g64), grad_bound(rel32)
    assert rel <= bound, f"{what}: rel-L2 vs fp64 {rel:.3e} > bound {bound:.3e} (fp32 reference: {rel32:.3e})"
    return rel / bound
