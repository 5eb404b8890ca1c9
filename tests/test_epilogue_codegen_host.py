"""Resources of the albedo sweeps and of the small-batch forward sweep, read from the generated code (tools/vm_trace.py: one
device-only compile of csrc/color_h2.hip and one of csrc/fused.hip with the library's flags; needs the compiler, no GPU).

The albedo backward once kept 35 values in scratch and reloaded them between its state stores; the forward epilogues now
hold their bias values across the matrix loop, which must not cost the small-batch kernel its fourth wave per SIMD.  What the
waits between the stores look like is left to the committed trace (profiles/epilogue_waits_codegen.txt)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("vm_trace", os.path.join(ROOT, "tools", "vm_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def color_kernels():
    return {k["name"]: k for k in _tool().kernels_of("color_h2").values()}


@pytest.fixture(scope="module")
def forward_kernels():
    return {k["name"]: k for k in _tool().kernels_of("fused", ["fused_forward_kernel"]).values()}


@pytest.mark.parametrize("name", ("color_fwd_h2_kernel", "color_bwd_h2_kernel"))
def test_albedo_sweeps_use_no_scratch_at_two_workgroups_per_cu(color_kernels, name):
    (k,) = [v for n, v in color_kernels.items() if name in n]
    assert k["res"]["scratch"] == 0, f"{name}: ScratchSize {k['res']['scratch']}"
    assert k["res"]["occupancy"] == 2, f"{name}: occupancy {k['res']['occupancy']} waves per SIMD"
    assert not any(t in ("sL", "sS") for _, b in k["blocks"] for t in b), f"{name}: scratch instructions in the trace"


def test_small_batch_forward_keeps_four_waves_per_simd(forward_kernels):
    (k,) = [v for n, v in forward_kernels.items() if "fused_forward_kernel<1, false, 8, true, true>" in n]
    assert k["res"]["occupancy"] == 4, f"occupancy {k['res']['occupancy']} waves per SIMD at {k['res']['vgprs']} VGPRs"
    assert k["res"]["scratch"] == 0
