"""The bf16 route's backward (RNB_VARIANT_BF16, csrc/bf16_*.hip) over the table of tests/bf16_point_matrix.py, on the device:
point counts M = rays x samples that end inside an 8-point K8 unit, inside either half of a 16-point MFMA step, and in a last
split of 1, 2, 3 or 5 chunks of bf_dw_kernel's LDS ring.

A. Every row is one train step against the bf16-emulating statement (tests/bf16_emu_step.py step: its bound rule, K = 4, its
   floors and caps, unchanged): every output, the loss and every gradient tensor; four rows again with deterministic=True (one
   block per head-backward kernel, ordered slabs).
B. The tail made to matter.  With sampled depths the last points of a batch lie behind the surface and carry almost no
   adjoint, so a dropped or doubled tail unit would move nothing.  Four rows run again at explicit depths
   (tests/bf16_point_matrix.py tail_case: a ray that hits the surface goes last, its last `tail` depths, the points of the last
   K8 unit, straddle the hit) with the last ray's loss weight set so that, in the fp64 emulation, that ray carries half of the
   norm of sdf.lin1.weight_v's gradient.  Same bound rule.  (The host test holds the recipe to >= 0.5 of the ray's `weights`
   on those points.)
C. Padded rows never reach a result: the step on buffers poisoned as in tests/test_gpu_parity.py
   test_uninitialised_workspace_is_never_read (fp32 NaN, 0xFF bytes) equals the clean step bit for bit, at M = 75 and 2772
   (Mp - M = 53 and 44), on the bf16 route (also with the fp32 albedo net behind it), the default arithmetic and f32_mfma.
D. The route, from the library's profiler: every bf16 case ran "dW(all)" once, the F / R / RA / FB sweeps, and no fp32 weight-
   gradient class.

Measured on MI355X, the worst device / emu32 ratio of each case over its gradient tensors | over its output rms and loss,
and the largest share of a bound any quantity of the case reaches (every ratio is printed: `pytest -s`, BF16EMU and BF16ROW
lines).  A ratio above K = 4 passes only under a floor: the quantity is then one or two flipped roundings.

  row (M)            default                deterministic          tail-heavy (share of the last ray's weights, fp64 oracle)
  1x22 (22)          4.55 | 4.84   0.81     4.55 | 4.84   0.81
  3x22 (66)          0.85 | 4.09   0.29                            0.58 | 1.45   0.30   (0.984)
  3x25 (75)          1.07 | 1.19   0.27     1.07 | 1.19   0.27     3.59 | 1.13   0.88   (0.981)
  172x16 (2752)      3.93 | 3.58   0.75
  126x22 (2772)      1.41 | 0.90   0.31     1.41 | 0.90   0.31     3.82 | 4.43   0.93   (0.764)
  502x11 (5522)      1.07 | 2.08   0.46     1.07 | 2.08   0.46     4.90 | 1.38   0.65   (0.954)
  3x22_no_albedo     0.23 | 4.09   0.29
  3x22_render        2.42 | 4.09   0.57     (its loss: 5.6e-6 against emu32's 3.1e-8, under the 2e-5 floor)
  3x25_mv6           1.04 | 3.69   0.39

M = 2752 and 5522 were first run as 86 x 32 and 251 x 22 rays x samples.  Each missed ONE tensor of the output layer (86 x 32:
sdf.lin8.bias 3.8e-4 against 1.8e-4; 251 x 22: sdf.lin8.weight_g 3.59e-4 against 3.54e-4, the same to three digits with
deterministic=True) while every output was within 1.1 x emu32's error.  That is rounding-flip noise the emulation's own fp32
orders show: on the same rays with depths sampled by the oracle, emu32 itself is 3.0e-4 (sdf.lin8.weight_g, 251 x 22) and
1.1e-4 .. 2.5e-4 (sdf.lin8.bias) from emu64, and on the device's depths it happened to be 6.3e-5 and 1.9e-5.  Both rows were
replaced by rows of the same M, hence the same classes, with more rays (172 x 16, 502 x 11); no bound changed.
"""
import ctypes as C
from dataclasses import replace

import pytest
import torch

from oracle import rnb_oracle as O
from tests import bf16_point_matrix as BM
from tests.bf16_emu_step import OUT_KEYS, step
from tests.golden_util import Golden
from tests.gpu_support import R  # noqa: F401
from tests.gpu_support import device, named

pytestmark = pytest.mark.gpu

BF16_SWEEPS = {"F_sweep(save)", "R_sweep", "RA_sweep", "FB_sweep"}
FP32_DW = {"dW(x3: 256x256 + narrow jobs)", "dW(slab reduce)"}       # (the fp32 albedo path's own jobs run as "dW(other)")


def profile_launches(R):
    """{kernel class: launches} of the library's profiler since rnb_profile_enable(1)"""
    lib = R.native.load()
    ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
    R.native.check(lib.rnb_profile_collect(C.byref(ms), C.byref(n), C.byref(fl)))
    buf = C.create_string_buffer(int(lib.rnb_profile_report(None, 0)) + 16)
    lib.rnb_profile_report(buf, len(buf))
    out = {}
    for ln in buf.value.decode().splitlines():
        tag, _, launches, _ = ln.rsplit(" ", 3)
        out[tag] = out.get(tag, 0) + int(launches)
    return out


def run_step(R, row, tag, **kw):
    """one step of tests/bf16_emu_step.py on `row` with the route assertion (D) and the BF16ROW line"""
    lib = R.native.load()
    info = {}
    sharpen = row.multires_view == 4        # (the sharpened fixture has the shipped albedo net; else a geometric init, seed 7)
    lib.rnb_profile_enable(1)
    try:
        n = step(R, row.model_conf, row.B, row.api, row.no_albedo, sharpen=sharpen, seed=2 if sharpen else 7,
                 tag=f"{tag} {row.name}", info=info, **kw)
        launches = profile_launches(R)
    finally:
        lib.rnb_profile_enable(0)
    print(f"BF16ROW {tag} {row.name}: M = {row.M}, Mp - M = {row.Mp - row.M}, splits {row.plan.splits} x {row.plan.rows} rows, last "
          f"{row.plan.last_rows}; worst device / emu32 {info['worst_ratio'][0]:.2f} ({info['worst_ratio'][1]}), worst share of a "
          f"bound {info['worst_of_bound'][0]:.2f} ({info['worst_of_bound'][1]}); last ray x {info['ray_weight']}; "
          f"launches {dict(sorted(launches.items()))}")
    assert launches.get("dW(all)") == 1, f"{tag} {row.name}: the grouped bf16 launch must run once: {launches}"
    assert BF16_SWEEPS <= set(launches), f"{tag} {row.name}: sweeps missing: {sorted(BF16_SWEEPS - set(launches))}"
    assert not (FP32_DW & set(launches)), f"{tag} {row.name}: an fp32 weight-gradient class ran: {launches}"
    if row.multires_view == 4:
        assert "dW(other)" not in launches, f"{tag} {row.name}: an fp32 weight-gradient class ran: {launches}"
    # every parameter the emulation has a gradient for: 3 per SDF layer, the variance, 3 per albedo layer
    mc = row.model_conf
    assert n == 3 * (mc.sdf.n_layers + 1) + 1 + (0 if row.no_albedo else 3 * (mc.color.n_layers + 1))
    return info


# ------------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("row", BM.ROWS, ids=[r.name for r in BM.ROWS])
def test_row_against_the_emulation(R, row):
    run_step(R, row, "default")


@pytest.mark.parametrize("name", BM.DETERMINISTIC_ROWS)
def test_deterministic_row_against_the_emulation(R, name):
    run_step(R, BM.BY_NAME[name], "deterministic", deterministic=True)


# ------------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("name", BM.TAIL_ROWS)
def test_tail_heavy_row_against_the_emulation(R, name):
    row = BM.BY_NAME[name]
    p = Golden("full_main_sharp").params()
    with torch.no_grad():
        p["dev.variance"].fill_(0.3)
    batch, z, pick = BM.tail_case(row, p)
    info = run_step(R, row, "tail", batch=batch, z_vals=z, tail_key=BM.TAIL_KEY)
    assert info["ray_weight"] > 0


# ------------------------------------------------------------------------------------------------------------------- C
def poisoned_pair(R, row, **variant):
    """the same deterministic step on clean and on poisoned torch.empty buffers: [(z_vals, outputs, gradients)] x 2"""
    mc = row.model_conf
    if row.multires_view == 4:
        p = Golden("full_main_sharp").params()
    else:
        torch.manual_seed(7)
        p = O.init_params(mc)
    batch = BM.row_batch(row)
    runs = []
    orig_empty, orig_empty_like = torch.empty, torch.empty_like

    def poison(t):
        if t.is_cuda and t.dtype == torch.float32:
            t.fill_(float("nan"))
        elif t.is_cuda and t.dtype == torch.uint8:
            t.fill_(255)
        return t

    for poisoned in (False, True):
        sdf, devn, col, ren = R.build_from_named_params(mc, {k: v.clone() for k, v in p.items()}, device())
        ren.set_variant(deterministic=True, **variant)
        b = {k: v.to(device()) for k, v in batch.items()}
        if poisoned:
            torch.empty = lambda *a, **k: poison(orig_empty(*a, **k))
            torch.empty_like = lambda *a, **k: poison(orig_empty_like(*a, **k))
        try:
            out = ren.render_rnb(b["rays_o"], b["rays_d"], b["near"], b["far"], b["lights_dir"], cos_anneal_ratio=1.0,
                                 t_rand=b["t_rand"])
            loss = O.rnb_loss(out, b["true_rgb"], b["mask"])[0]
            loss.backward()
            torch.cuda.synchronize()
        finally:
            torch.empty, torch.empty_like = orig_empty, orig_empty_like
        grads = {k: v.grad.clone() for k, v in named(sdf, devn, col).items()}
        runs.append((ren.last_z_vals.clone(), {k: v.detach().clone() for k, v in out.items()}, grads))
    return runs


def assert_bit_equal(runs, tag):
    (z0, o0, g0), (z1, o1, g1) = runs
    assert tuple(z0.shape)[0] * tuple(z0.shape)[1] % BM.K8 != 0, "the row must end inside a K8 unit"
    assert torch.equal(z0, z1), f"{tag}: z_vals depend on what the buffers held before the call"
    for k in OUT_KEYS:
        assert bool(torch.isfinite(o0[k]).all()), f"{tag}: output {k} of the clean run is not finite"
    for k in o0:
        assert torch.equal(o0[k], o1[k]), f"{tag}: output {k} depends on what its buffers held before the call"
    for k in g0:
        assert bool(torch.isfinite(g0[k]).all()), f"{tag}: gradient of {k} of the clean run is not finite"
        assert torch.equal(g0[k], g1[k]), f"{tag}: gradient of {k} depends on what the workspace held before the call"
    assert float(g0[BM.TAIL_KEY].abs().max()) > 0


@pytest.mark.parametrize("variant", [dict(bf16=True), dict(), dict(f32_mfma=True)], ids=["bf16", "default", "f32_mfma"])
@pytest.mark.parametrize("name", BM.POISON_ROWS)
def test_padded_rows_never_reach_a_result(R, name, variant):
    assert_bit_equal(poisoned_pair(R, BM.BY_NAME[name], **variant), f"{name} {variant}")


@pytest.mark.parametrize("name", BM.POISON_ROWS)
def test_padded_rows_never_reach_a_result_behind_the_fp32_albedo_net(R, name):
    """multires_view = 6: FB reads the fp32 fbar the fp32 albedo backward left, padded rows included"""
    assert_bit_equal(poisoned_pair(R, replace(BM.BY_NAME[name], multires_view=6), bf16=True), f"{name} multires_view=6 bf16")
