"""Host-side checks of the render's input gradients (RNB_FLAG_INPUT_GRADS, rnb_render_bwd_inputs): the workspace query, the
refusals that come before any device work, and the binding."""
import ctypes as C

import pytest

import rnb_neus_fork_amd as R

N = R.native


def _desc(variant=0, **shape):
    kw = dict(sdf_hidden=256, n_layers=8, multires=6, d_out=257)
    kw.update(shape)
    sdf = R.SDFNetwork(d_in=3, d_out=kw["d_out"], d_hidden=kw["sdf_hidden"], n_layers=kw["n_layers"],
                       skip_in=[4] if kw["n_layers"] > 4 else [], multires=kw["multires"])
    col = R.RenderingNetwork(d_feature=kw["d_out"] - 1, mode="no_view_dir", d_in=6, d_out=3, d_hidden=256, n_layers=2,
                             multires_view=4)
    d = R.model_desc(sdf, col)
    d.variant = variant
    return d


def _ws(d, B, S, flags):
    b = C.c_int64()
    N.check(N.load().rnb_render_workspace_bytes(C.byref(d), B, S, flags, C.byref(b)))
    return b.value


def test_flag_value_and_binding():
    assert N.FLAG_INPUT_GRADS == 32
    assert "rnb_render_bwd_inputs" in N.EXPORTED_SYMBOLS
    assert [f[0] for f in N.RenderInputGrads._fields_] == ["rays_o", "rays_d", "lights_dir", "background_rgb", "z_vals"]
    assert C.sizeof(N.RenderInputGrads) == 5 * C.sizeof(C.c_void_p)
    assert hasattr(N.load(), "rnb_render_bwd_inputs")


@pytest.mark.parametrize("shape", [dict(), dict(sdf_hidden=64, n_layers=2, multires=0, d_out=33)])
def test_workspace_with_the_flag_is_never_smaller(shape):
    d = _desc(**shape)
    for B, S in ((1, 2), (64, 32), (512, 128), (4096, 128)):
        for mode in (N.MODE_CORE, N.MODE_MVPS, N.MODE_MVPS | N.FLAG_LIGHT_PER_RAY | N.FLAG_RELU_SHADING,
                     N.MODE_MVPS | N.FLAG_NO_ALBEDO):
            base = _ws(d, B, S, mode)
            assert _ws(d, B, S, mode | N.FLAG_INPUT_GRADS) > base
            assert _ws(d, B, S, mode | N.FLAG_FORWARD_ONLY) <= base   # (unchanged: the flag adds state, nothing else moves)


def test_bf16_with_the_flag_is_refused_with_a_message():
    d = _desc(variant=N.VARIANT_BF16)
    lib = N.load()
    b = C.c_int64()
    N.check(lib.rnb_render_workspace_bytes(C.byref(d), 512, 128, N.MODE_MVPS, C.byref(b)))   # without: as before
    rc = lib.rnb_render_workspace_bytes(C.byref(d), 512, 128, N.MODE_MVPS | N.FLAG_INPUT_GRADS, C.byref(b))
    assert rc == -1
    assert b"RNB_VARIANT_BF16" in lib.rnb_last_error_string()


def _bwd_inputs(d, flags, **want):
    """rnb_render_bwd_inputs with placeholder pointers: every case here is refused before anything is dereferenced."""
    lib = N.load()
    args = N.RenderArgs()
    args.B, args.S, args.n_lights, args.flags = 4, 8, 1, flags
    gout = N.RenderGrads()
    ig = N.RenderInputGrads()
    for k, v in want.items():
        setattr(ig, k, v)
    fake = C.c_void_p(256)
    return lib.rnb_render_bwd_inputs(C.byref(d), fake, C.byref(args), C.byref(gout), C.byref(ig), fake, fake, fake,
                                     1 << 20, None)


def test_refusals_of_rnb_render_bwd_inputs():
    lib = N.load()
    msg = lambda: lib.rnb_last_error_string().decode()
    assert _bwd_inputs(_desc(variant=N.VARIANT_BF16), N.MODE_MVPS | N.FLAG_INPUT_GRADS, rays_o=256) == -1
    assert "RNB_VARIANT_BF16" in msg()
    d = _desc()
    assert _bwd_inputs(d, N.MODE_MVPS, rays_o=256) == -1 and "RNB_FLAG_INPUT_GRADS" in msg()
    assert _bwd_inputs(d, N.MODE_MVPS, lights_dir=256) == -1 and "RNB_FLAG_INPUT_GRADS" in msg()
    assert _bwd_inputs(d, N.MODE_CORE | N.FLAG_INPUT_GRADS, lights_dir=256) == -1 and "RNB_MODE_CORE" in msg()
    assert _bwd_inputs(d, N.MODE_MVPS | N.FLAG_INPUT_GRADS, background_rgb=256) == -1 and "background" in msg()
    assert _bwd_inputs(d, N.MODE_CORE | N.FLAG_INPUT_GRADS, background_rgb=256) == -1 and "background" in msg()
