"""The kernel variants of the 256-wide network, as (id, NeuSRenderer.set_variant keywords).

A plain module: tests/test_gpu_parity.py runs every one against the golden fp64 values, tests/test_gpu_guard_render.py between
guard bands."""
# the kernel variants of the 256-wide network (rnb_model_desc.variant): RNB_VARIANT_GENERIC forces the per-layer GEMM
# path, DW_LDS / DW_STAGED the other weight-gradient kernels, the BWD_TI / BWD_NW / FWD_TI / FWD_NW bits the other tile
# shapes of the sweeps, F32_MFMA the native fp32 MFMA, x2h=False the six-bf16-term forward sweeps, reg_tile the M/V kernels
VARIANTS = (("fused", {}), ("generic", dict(generic=True)), ("dw_lds", dict(dw_lds=True)),
            ("dw_staged", dict(dw_staged=True)), ("dw_staged_det", dict(dw_staged=True, deterministic=True)),
            ("bwd_ti1", dict(bwd_ti=1, bwd_nw=4)), ("bwd_ti2", dict(bwd_ti=2, bwd_nw=4)),
            ("bwd_ti2_nw8", dict(bwd_ti=2, bwd_nw=8)), ("fwd_ti1", dict(fwd_ti=1, fwd_nw=4)),
            ("deterministic", dict(deterministic=True)), ("x3", dict(x3=True)),
            ("fwd_ti2_nw8", dict(fwd_ti=2, fwd_nw=8)), ("f32_mfma", dict(f32_mfma=True)), ("f32_mfma_ti2", dict(f32_mfma=True, bwd_ti=2, bwd_nw=4)),
            ("x3_ti1_nw4", dict(x3=True, bwd_ti=1, bwd_nw=4, fwd_ti=1, fwd_nw=4)),
            ("x3_ti2_nw8", dict(x3=True, bwd_ti=2, bwd_nw=8, fwd_ti=2)),
            ("no_x2h", dict(x2h=False)), ("no_x2h_det", dict(x2h=False, deterministic=True)),
            ("x2h_ti1", dict(x2h=True, bwd_ti=1, bwd_nw=4, fwd_ti=1, fwd_nw=4)),
            ("x2h_reg_tile", dict(x2h=True, reg_tile=True)))
