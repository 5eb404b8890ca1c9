"""Host-side checks of the opt-in autograd of the direct network calls (SDFNetwork / RenderingNetwork.set_autograd): the
default stays the loud forward-only guard, the opt-in is a plain attribute, and the workspace query of the differentiable
point calls (rnb_points_grad_workspace_bytes) works without a device."""
import ctypes as C

import pytest
import torch

import rnb_neus_fork_amd as R


def _nets():
    sdf = R.SDFNetwork(d_in=3, d_out=33, d_hidden=32, n_layers=2, skip_in=[], multires=2)
    col = R.RenderingNetwork(d_feature=32, mode="no_view_dir", d_in=6, d_out=3, d_hidden=32, n_layers=1, multires_view=2)
    return sdf, col


def _calls(sdf, col, x):
    return (lambda: sdf(x), lambda: sdf.sdf(x), lambda: sdf.sdf_hidden_appearance(x), lambda: sdf.gradient(x),
            lambda: col(x, x, x, torch.zeros(4, 32)))


def test_flag_off_keeps_the_forward_only_guard():
    sdf, col = _nets()
    x = torch.zeros(4, 3)
    for call in _calls(sdf, col, x):
        with pytest.raises(RuntimeError, match="forward-only.*NeuSRenderer.render.*set_autograd\\(True\\)"):
            call()
    sdf.set_autograd(True).set_autograd(False)
    col.set_autograd(False)
    for call in _calls(sdf, col, x):
        with pytest.raises(RuntimeError, match="forward-only"):
            call()


def test_flag_on_with_cpu_tensors_asks_for_the_gpu():
    sdf, col = _nets()
    sdf.set_autograd(True)
    col.set_autograd(True)
    x = torch.zeros(4, 3)
    for call in _calls(sdf, col, x):
        with pytest.raises(RuntimeError, match="must live on the GPU") as e:
            call()
        assert "forward-only" not in str(e.value)
    # an input that requires grad, frozen parameters: still the differentiable call
    for q in list(sdf.parameters()) + list(col.parameters()):
        q.requires_grad_(False)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        sdf.sdf(x.clone().requires_grad_(True))


def test_set_autograd_returns_the_module_and_leaves_the_state_dict_alone():
    sdf, col = _nets()
    keys_s, keys_c = list(sdf.state_dict().keys()), list(col.state_dict().keys())
    assert sdf.set_autograd() is sdf and col.set_autograd(True) is col
    assert sdf._autograd is True and col._autograd is True
    assert list(sdf.state_dict().keys()) == keys_s and list(col.state_dict().keys()) == keys_c
    assert sdf.to(torch.float32)._autograd is True   # a plain attribute survives .to()
    assert "_autograd" not in dict(sdf.named_buffers())
    # a fresh module: off
    assert not getattr(_nets()[0], "_autograd", False)


def _desc(sdf_hidden=256, n_layers=8, multires=6, d_out=257):
    sdf = R.SDFNetwork(d_in=3, d_out=d_out, d_hidden=sdf_hidden, n_layers=n_layers, skip_in=[4] if n_layers > 4 else [],
                       multires=multires)
    col = R.RenderingNetwork(d_feature=d_out - 1, mode="no_view_dir", d_in=6, d_out=3, d_hidden=256, n_layers=2,
                             multires_view=4)
    return R.model_desc(sdf, col)


def _grad_ws(d, n, flags):
    b = C.c_int64()
    R.native.check(R.native.load().rnb_points_grad_workspace_bytes(C.byref(d), n, flags, C.byref(b)))
    return b.value


def _points_ws(d, n):
    b = C.c_int64()
    R.native.check(R.native.load().rnb_points_workspace_bytes(C.byref(d), n, C.byref(b)))
    return b.value


@pytest.mark.parametrize("shape", [dict(), dict(sdf_hidden=64, n_layers=2, multires=0, d_out=33)])
def test_grad_workspace_query_on_the_host(shape):
    lib = R.native.load()
    d = _desc(**shape)
    b = C.c_int64()
    with pytest.raises(R.native.NativeError, match="n_points < 0"):
        R.native.check(lib.rnb_points_grad_workspace_bytes(C.byref(d), -1, 0, C.byref(b)))
    with pytest.raises(R.native.NativeError, match="unknown bits"):
        R.native.check(lib.rnb_points_grad_workspace_bytes(C.byref(d), 10, 64, C.byref(b)))
    F, N, Col = R.native.POINTS_FEATURE, R.native.POINTS_NORMAL, R.native.POINTS_COLOR
    for n in (1, 63, 4097, 100_000):
        base = _grad_ws(d, n, 0)
        assert base >= _points_ws(d, n)
        for fl in (F, N, F | N):
            assert _grad_ws(d, n, fl) >= _points_ws(d, n)
        # each flag adds state; strictly so where the differentiable state exceeds the forward-only calls' workspace
        # (the shipped shape; a small SDF net behind a 256-wide albedo net sits on that floor without the normal)
        grow = (lambda a, b: a > b) if not shape else (lambda a, b: a >= b)
        assert grow(_grad_ws(d, n, F), base) and grow(_grad_ws(d, n, N), base)
        assert grow(_grad_ws(d, n, F | N), _grad_ws(d, n, N)) and grow(_grad_ws(d, n, F | N), _grad_ws(d, n, F))
        assert _grad_ws(d, n, Col) >= base
    for fl in (0, F, N, F | N, Col):
        assert _grad_ws(d, 4097, fl) > _grad_ws(d, 63, fl) >= _grad_ws(d, 1, fl)   # (rows pad to 128)
        assert _grad_ws(d, 100_000, fl) > _grad_ws(d, 4097, fl)
    assert _grad_ws(d, 0, 0) >= 0
